"""The six load_yaml* functions of the package over their one private loader: each one's return tuple, the name its errors
carry, and that `path` loads what `text` loads. The keys themselves are pinned by the test_host_* file of each feature; what
every entry point of the library answers for the corpus of tests/yaml_loader_cases.py is pinned by a recorded file. No GPU."""
import pytest

from yaml_loader_cases import GOLDEN, LOADERS, MOTION, SCENE, parse, run_corpus, serialize


def _describe(rtc, name, result):
    """The tuple as comparable values: the shapes' and lights' bytes, the camera's, and each extra as its bytes / value."""
    w, cam, *extra = result
    assert len(extra) == len(LOADERS[name][2])
    out = [[bytes(s) for s in w.shapes], [bytes(l) for l in w.lights], bytes(cam)]
    for what, v in zip(LOADERS[name][2], extra):
        out.append(v if what == "samples" else [bytes(m) for m in v] if what == "motions" else None if v is None else bytes(v))
    return out


@pytest.mark.parametrize("name", sorted(LOADERS))
def test_tuple_path_and_error_name(rtc, name, tmp_path):
    load = getattr(rtc, name)
    where, keys, parts = LOADERS[name]
    text = SCENE % (keys, MOTION if name == "load_yaml_motion" else "")
    got = load(text=text)
    w, cam, *extra = got
    assert len(w) == 2 and len(w.lights) == 2 and (cam.hsize, cam.vsize) == (40, 30)
    for what, v in zip(parts, extra):
        if what == "lens":
            assert (v.aperture, v.focal_distance) == (0.1, 7.0)
        elif what == "ao":
            assert v.radius == 0.75
        elif what == "gather":
            assert v.radius == 2.0
        elif what == "no lens":
            assert v is None
        elif what == "projection":
            assert v.width == 4.0
        elif what == "motions":
            assert len(v) == 1 and v[0].shape == 0
        else:
            assert v == 3
    # absent keys: the optional parts are None, no motions, one shutter sample
    _, _, *bare = load(text=SCENE % ("", ""))
    assert bare == [[] if what == "motions" else 1 if what == "samples" else None for what in parts]
    # `path` calls the entry point's _file twin: the same scene
    f = tmp_path / "scene.yml"
    f.write_text(text)
    assert _describe(rtc, name, load(path=f)) == _describe(rtc, name, got)
    # a failure carries the status, the function's name and the library's message
    for kwargs, detail in (({"text": SCENE % ("", "    - [bogus, 1]")}, "unknown transform: bogus"), ({"path": tmp_path / "absent.yml"}, "")):
        with pytest.raises(rtc.RtcError) as e:
            load(**kwargs)
        assert e.value.status != 0 and str(e.value).startswith(where + ": ") and detail in str(e.value), (name, str(e.value))


def test_recorded_corpus_through_every_entry_point(rtc, tmp_path):
    """Every document of tests/yaml_loader_cases.py through the 24 YAML and the 6 Lua entry points of rtc.lib(): status,
    message and a hash of every out-argument (buffers filled with 0xA5 before the call), against the answers recorded from
    the loader as it stood before its entry points shared one request record (tests/golden/scene_loader_results.txt)."""
    import sys
    want = parse(GOLDEN.read_text())
    got = run_corpus(rtc.lib(), sys.modules[rtc.__name__ + ".abi"], tmp_path)
    assert [name for name, _ in got] == list(want), "the corpus itself changed: its documents are not the recorded ones"
    calls = [answer for _, rows in got for _, answer in rows]
    # most of the equality would be vacuous if the corpus were mostly refused, or mostly accepted
    assert 3 * sum(st == 0 for st, _, _ in calls) >= len(calls) and 3 * sum(st == 5 for st, _, _ in calls) >= len(calls)
    differ = [f"{name!r} through {fn}: (status, message, hash) {answer}, recorded {rec}"
              for name, rows in got for (fn, answer), rec in zip(rows, want[name]) if answer != rec]
    assert not differ and all(len(rows) == len(want[name]) for name, rows in got), f"{len(differ)} calls differ:\n" + "\n".join(differ[:20])
    assert serialize(got) == GOLDEN.read_text()
