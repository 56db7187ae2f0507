"""The six load_yaml* functions of the package over their one private loader: each one's return tuple, the name its errors
carry, and that `path` loads what `text` loads. The keys themselves are pinned by the test_host_* file of each feature. No GPU."""
import pytest

SCENE = """
- add: camera
  width: 40
  height: 30
  field-of-view: 0.8
  from: [0, 2, -6]
  to: [0, 1, 0]
  up: [0, 1, 0]
%s
- add: light
  at: [-5, 8, -5]
  intensity: [1, 1, 1]
- add: light
  at: [5, 8, -5]
  intensity: [0.5, 0.5, 0.5]
- add: sphere
  transform:
    - [translate, 0, 1, 0]
%s
- add: plane
"""
LENS = "  aperture: 0.1\n  focal-distance: 7\n"
MOTION = "  motion:\n    - [translate, 1, 0, 0]"

# function -> (the name its errors carry, the camera keys of the scene it is given, what follows (World, camera) in its tuple)
LOADERS = {
    "load_yaml": ("rtc_scene_load_yaml", "", ()),
    "load_yaml_lens": ("rtc_scene_load_yaml_lens", LENS, ("lens",)),
    "load_yaml_ao": ("rtc_scene_load_yaml_ao", LENS + "  ao-radius: 0.75", ("lens", "ao")),
    "load_yaml_gather": ("rtc_scene_load_yaml_gather", LENS + "  ao-radius: 0.75\n  gather-radius: 2", ("lens", "ao", "gather")),
    "load_yaml_projection": ("rtc_scene_load_yaml_projection", "  projection: orthographic\n  ortho-width: 4", ("no lens", "projection")),
    "load_yaml_motion": ("rtc_scene_load_yaml_motion", LENS + "  shutter-samples: 3", ("lens", "motions", "samples")),
}


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
