"""Runs tests/cpp/test_facade_resize.cpp — the C++ mirror's resize (Canvas::resized) — on the GPU, as the sibling facade tests
run theirs: the program is prebuilt by build()."""
import importlib.util
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def _build():
    spec = importlib.util.spec_from_file_location("_rtc_build", ROOT / "raytracer-challenge_amd" / "build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


@pytest.mark.gpu
def test_facade_resize(rtc):
    exe = _build().build_facade_resize_test()
    assert exe is not None and exe.exists()
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "facade resize: ok" in r.stdout
