"""The candidate-list cases on the CPU (tests/candidate_list_cases.py): every case builds deterministically, names a
decision, and meets its own CPU-side expectation on the oracle's canvas and hit records — lit and shadowed floor pixels
both present, hit points on both sides of the light lists' reach, shadow origins beyond the prefilter limit, directions
on a cube-map face border, Camera::render's untraced row and column black."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))
K = __import__("candidate_list_cases").sibling("candidate_list_cases")     # (one copy per process: the helper's own loader)
CASES = K.all_cases()

DECISIONS = ("tile_cap", "n_unb_limit", "plane_pose", "plane_oy_guard", "plane_rr_guard", "unbounded_non_plane", "cone_off",
             "cone_narrow", "camera_pose", "frame_edges", "light_n", "light_cap", "light_reach", "light_many_cells",
             "light_position", "light_face_border", "light_pre_ok", "light_occluder", "light_secondary")


def test_every_decision_has_a_case_and_names_are_unique():
    assert {c.decision for c in CASES} == set(DECISIONS)
    assert len({c.name for c in CASES}) == len(CASES)
    assert all(c.expect is not None for c in CASES if c.name != "frame[1x9]")
    # the counts the cases are for: lists from 32 objects, the small cap up to 256, both caps met exactly and exceeded by one
    by = {c.name: c for c in CASES}
    assert [by[f"light_count[{n}]"].cap for n in (31, 32, 33, 256, 257, 320, 321)] == [0, 16, 16, 16, 128, 128, 128]
    assert [by[f"light_cell_cap[{k}]"].want["cell"][1] - by[f"light_cell_cap[{k}]"].cap for k in (16, 17, 128, 129)] == [0, 1, 0, 1]
    assert [by[f"tile_cap[{k}]"].want["tile"][2] - K.TILE_CAP for k in (63, 64, 65, 66)] == [-1, 0, 1, 2]


def test_cases_build_deterministically():
    again = K.all_cases()
    assert [c.name for c in again] == [c.name for c in CASES]
    for a, b in zip(CASES, again):
        assert a.n == b.n and bytes(a.arr()) == bytes(b.arr()) and bytes(a.light) == bytes(b.light) and bytes(a.cam) == bytes(b.cam), a.name
    for size in ("small", "large"):
        s1, l1, c1 = K.list_world(5, size)
        s2, l2, c2 = K.list_world(5, size)
        assert len(s1) == len(s2) and all(bytes(x) == bytes(y) for x, y in zip(s1, s2)) and bytes(l1) == bytes(l2) and bytes(c1) == bytes(c2)
        assert (32 <= len(s1) <= 256) if size == "small" else (257 <= len(s1) <= 1500)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_meets_its_cpu_expectation(O, case):
    canvases = {m: O.render(case.arr(), case.n, case.light, case.cam, mode=m, nthreads=8) for m in case.modes}
    for img in canvases.values():
        assert np.isfinite(img).all(), case.name
    if case.expect is not None:
        case.expect(case, canvases)


def test_the_seeded_family_is_finite_and_varied(O):
    """Every 8th seed of the small class and seed 0 of the large one render finite on the oracle; over the 40 seeds the
    family draws planes in every count 0..6, and both the wide-angle and the far-away variant."""
    planes, wide, far = set(), 0, 0
    for size in ("small", "large"):
        for seed in range(40):
            shapes, lgt, cam = K.list_world(seed, size)
            planes.add(sum(1 for s in shapes if s.kind == K.PLANE))
            wide += cam.half_width > 5.
            far += abs(lgt.position[0]) > 1e5
            if seed % 8 == 0 and (size == "small" or seed == 0):
                a = (O.RtcShape * len(shapes))(*shapes)
                assert np.isfinite(O.render(a, len(shapes), lgt, cam, mode=1, nthreads=8)).all(), (size, seed)
    assert planes == set(range(7)) and wide > 0 and far > 0
