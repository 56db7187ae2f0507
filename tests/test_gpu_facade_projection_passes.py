"""tests/cpp/test_facade_projection_passes.cpp: ch1::Camera::render_aov / render_async_aov / render_ao / render_gather with an
explicit rtc_projection give the planes of rtc_render_aov_projection, rtc_render_ao_projection and
rtc_render_gather_projection; the forms without the argument still throw while a projection is set on the camera; a lens or a
shutter is refused. Built and run as the other facade programs are."""
import importlib.util
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


def test_facade(rtc):
    spec = importlib.util.spec_from_file_location("_rtc_build", ROOT / "raytracer-challenge_amd" / "build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    exe = b.build_facade_projection_passes_test()
    assert exe is not None and exe.exists()
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "facade projection passes: ok" in r.stdout
