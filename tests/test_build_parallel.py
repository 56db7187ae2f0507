"""build.py's compile loop, driven with a stand-in compiler (no hipcc, no GPU): the job count and its cap, every object
made before the link, compiles that overlap, staleness against every csrc/*.h, and a failing compile raised with that
compiler's output."""
import importlib.util
import os
import stat
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

# writes its -o file, or fails for the sources named in $FAIL; keeps a log of what it was asked to do. A source named in
# $MEET says so in $MEET_DIR and goes on only when every source of $MEET has: two of them need two compilers at once.
COMPILER = """#!/bin/sh
for a in "$@"; do
  for f in $FAIL; do case "$a" in */$f) echo "$f: error: refused"; exit 1;; esac; done
  for f in $MEET; do case "$a" in */$f)
    : > "$MEET_DIR/$f"
    for g in $MEET; do n=0; until [ -e "$MEET_DIR/$g" ]; do n=$((n+1)); [ $n -gt 500 ] && { echo "$f: alone"; exit 1; }; sleep 0.01; done; done;;
  esac; done
done
while [ $# -gt 0 ]; do
  case "$1" in -shared) echo link >> "$LOG";; -c) echo "compile $2" >> "$LOG";; -o) : > "$2";; esac
  shift
done
"""


@pytest.fixture
def build(tmp_path, monkeypatch):
    cc = tmp_path / "cc"
    cc.write_text(COMPILER)
    cc.chmod(cc.stat().st_mode | stat.S_IXUSR)
    monkeypatch.setenv("HIPCC", str(cc))
    monkeypatch.setenv("LOG", str(tmp_path / "log"))
    monkeypatch.setenv("FAIL", "")
    monkeypatch.setenv("MEET", "")
    monkeypatch.setenv("MEET_DIR", str(tmp_path))
    spec = importlib.util.spec_from_file_location("_rtc_build_under_test", ROOT / "raytracer-challenge_amd" / "build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.ROOT, b.LIB = tmp_path, tmp_path / "librtc.so"  # objects and library go to the test's own directory
    return b


def test_job_count_is_max_jobs_or_the_cpu_count_and_at_most_16(build, monkeypatch):
    for value, want in (("3", 3), ("16", 16), ("40", 16), ("1", 1)):
        monkeypatch.setenv("MAX_JOBS", value)
        assert build.jobs() == want
    monkeypatch.delenv("MAX_JOBS")
    assert build.jobs() == min(16, os.cpu_count() or 1)


def test_every_source_is_compiled_and_the_link_comes_last(build, tmp_path):
    assert set(build.KERNEL_SOURCES) <= set(build.SOURCES) and len(set(build.SOURCES)) == len(build.SOURCES)
    assert all((build.CSRC / name).exists() for name in build.SOURCES)
    assert build.build(force=True) == tmp_path / "librtc.so"
    log = (tmp_path / "log").read_text().split("\n")[:-1]
    assert log[-1] == "link" and log.count("link") == 1
    assert sorted(log[:-1]) == sorted(f"compile {build.CSRC / name}" for name in build.SOURCES)
    assert all((tmp_path / "build" / "rtc" / (name + ".o")).exists() for name in build.SOURCES)


def test_two_compilers_run_at_once(build, tmp_path, monkeypatch):
    monkeypatch.setenv("MAX_JOBS", "2")
    monkeypatch.setenv("MEET", " ".join(build.SOURCES[:2]))  # each waits for the other to have started: serial compiles never meet
    build.build(force=True)
    assert (tmp_path / "log").read_text().count("compile ") == len(build.SOURCES)


def test_a_source_is_stale_against_every_header_in_csrc(build, tmp_path):
    """include/rtc.h and csrc/*.h by glob: a header nobody listed still makes every object stale."""
    build.CSRC = tmp_path / "csrc"
    build.CSRC.mkdir()
    (tmp_path / "include").mkdir()
    for f in [tmp_path / "include" / "rtc.h", build.CSRC / "old.h", *(build.CSRC / name for name in build.SOURCES)]:
        f.write_text("")
    compiles = lambda: (tmp_path / "log").read_text().count("compile ")
    build.build()
    assert compiles() == len(build.SOURCES)
    build.build()
    assert compiles() == len(build.SOURCES)  # nothing stale, nothing compiled
    newer = (tmp_path / "librtc.so").stat().st_mtime + 10.0
    (build.CSRC / "new.h").write_text("")
    os.utime(build.CSRC / "new.h", (newer, newer))
    build.build()
    assert compiles() == 2 * len(build.SOURCES)
    for f in [tmp_path / "librtc.so", *(tmp_path / "build" / "rtc").iterdir()]:
        os.utime(f, (newer + 5.0, newer + 5.0))  # (built after the header, whose time lies ahead of the clock)
    os.utime(build.CSRC / build.SOURCES[3], (newer + 10.0, newer + 10.0))  # one source alone: one compile
    build.build()
    assert compiles() == 2 * len(build.SOURCES) + 1


def test_a_failing_compile_raises_with_that_compilers_output(build, tmp_path, monkeypatch):
    monkeypatch.setenv("FAIL", "host_ppm.cpp")
    with pytest.raises(subprocess.CalledProcessError) as err:
        build.build(force=True)
    assert str(build.CSRC / "host_ppm.cpp") in err.value.cmd and err.value.output == "host_ppm.cpp: error: refused\n"
    assert "link" not in (tmp_path / "log").read_text().split("\n") and not (tmp_path / "librtc.so").exists()
