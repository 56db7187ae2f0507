"""CPU only: the hostile worlds of tests/adversarial_worlds.py are what they claim to be.

1. The moved generators build, seed by seed, the bytes they built before the move (SHA-256 of the shape records, the first
   light and the camera, recorded at the commit before the move).
2. Every helper is deterministic in its seed, finite, and leaves every shape invertible by the oracle's determinant rule.
3. Every case of the table the GPU tests read is of its class (materials, object count, lights, straddling lens origins,
   a near_surface light wider than a cone, penumbra counts) and its oracle reference has lit, shadowed and black pixels,
   so no GPU case can pass vacuously.
4. The table names exactly the cells of the instantiation matrix."""
import json

import numpy as np
import pytest

import adversarial_worlds as A

DIGESTS = json.loads("""
{
 "adversarial_scene": {
 "1000": "c52ba32d49d944c097e9069e131757e415b54cd996f3747298d0d18852c634bf",
 "1001": "6033b0dba6f5b02a022fa8192b10f3025da59b4b478ed98528b33f3e23a7418d",
 "1002": "30942f1cec0e7cc9dfcc110d0d2bcd9d3522d7fb10489175a4e71253a5bd958e",
 "1003": "0ff93a43786bdd484ce98bb6175d00be26c7d13614ed56f265ff0696d2b58bb2",
 "1004": "31f5cd5166047c6a4bdb0c6bc26988bb333b15d9b743ae608fbfde57a2c9a79d",
 "1005": "4f0864a3b927f768d8e549dbf311e650b715e41472c317c2837ca42e04f89d82",
 "1006": "5f2f42d5df4f2208f4e6c7da2d91e657f06a13088abf807b9a5a3c310279f8dc",
 "1007": "97d9799b7ece9808a181340e752c0866b0cd5571517e193b3a12a94776523902",
 "1008": "27422f480c1547284b09fb0d9a3595adb328e91bdd98c9d171cf24531a9d772a",
 "1009": "9a7e740d2d9f3ddc92f6fc15959de4c848b5b685cd0cb7230b807ef937eeabae",
 "1010": "ee171285a7edcbad091b21dd63a3b2bce785dc91d180e330360deff3878a06fe",
 "1011": "bfd98e74d880d6a126635ffea1c760ec5b405f8c33925c5ee245ca7a99b47df3",
 "1012": "2f9b2e0858bbef6f5c1385ea95ecc626d82c744777dbb3b5e3d93578222144be",
 "1013": "c325abfa1e7588690736a1d83accd4002fb1a967b12f0826a9aedd0d5fdff4a8",
 "1014": "98c3327c85038d8520e8a712cd910810eac263fe2ddcf8114791dace97835359",
 "1015": "91b4bc638713ed822002bf6a26e52325186773e16519f68bcc2b92c0cd8ee7fd",
 "1016": "6f9ceac6fdbe3f470bb214b2bbd8171b463e62d93eb22e5ebf77aada3c76e2b1",
 "1017": "2e2e89455f6976a20114c83e6b8ff2a248df657c73d07e22e14f04da2874b57f",
 "1018": "3f82c3df1adf29a38a69520567d99df48974eeb293f651f40e55bd6be85f0242",
 "1019": "cd194e8ebb63fab7a74daa64f75c1f2fd6c3cac06111f5045d1d68613563c377",
 "1020": "54449a0e25f554194ae7a8436bcb3c2f010804375d668b37ddbe3cfe6821e907",
 "1021": "0740cf16745559e65b72d6f66f3f2eb42d29c67f86cd5ab2767a2f8fe33632d1",
 "1022": "20c29d107bbeafd16097f25235f56c94f17a07f0eff48451fc8c2349f89678b9",
 "1023": "f97a0974389b4040226ff849c37c923856e8c4feba031cd067202dab99821052",
 "1024": "8fa4a1cef9898906b2aa044099263acb73184beb22d1cb55cc4d17ae7b3b3279",
 "1025": "5b1f7025e25eb6e1d1a082f92d508646d928dd723792da04c5c1b5abe279adec",
 "1026": "a61be859ec98437bfd4dea951c925efc68101cf4dddff1be1742d440000346b0",
 "1027": "3609ef17cf39220f5e3d491791b1d0f6b192cb2689c66fffb248d94eb814e78d",
 "1028": "855ae23b67fe6f42ec7cd46218002b75db2ec18278ddc3d530b0e6f8eef9ed1d",
 "1029": "a6c484327e98cc893037d787f1f8b2b5671f2a1159454601dd47f2dd6bbf7cac",
 "1030": "a4a9b6c38f33d4b24a0a02e2ffa09a8ea74c925da73a8b9de32f7df42d9a0012",
 "1031": "0da1dc70d3be4e4f66a6615424a6898c6cc309eae4fa9b0fbdac3df5ff36ea58",
 "1032": "5d7911bd75a5ad8f092df8fdf9eff054f171e58210e5adfa0235a6f6aed59321",
 "1033": "627cf4fa57c7b98ecd9a6d73b4c1f543b6c9631ddfd3b4e00217ea975803b43a",
 "1034": "b17290f5fde3ec714197a25ae4afb8d6ffce5c452702e9e37ac61cabc4ef432b",
 "1035": "3b5f08c7e5a1ca16619cd79a5ec6e8632bfe57d7a4d35034b1f1c07084c670c1",
 "1036": "c73ec6c849e4f6263c5e9bee9da346db2f7941bd8839cd9d6477dad11628fd8e",
 "1037": "7360eef3abdb9922d447850d7c8252bdfe960fd2893e6ea7fb763f9cf006f3e8",
 "1038": "e28031439696fced8fb157db4b049cb4c2a2ef6f3b37d6a5a582dc0dc7715e98",
 "1039": "2f066dd72a77a006b0f43cad5fd818cdf831df77a7b071fa1b3ff3d0e54ee793",
 "701683": "b5a879a4cb9a28bbc667dc6f7dab074aae56026e4b22e1fbb5b0a57df2e81368",
 "755117": "46c5a7cb4dddb4975a365b2a6ee11873cfcaac69b316066fbc0a47e98cc160d2"
},
 "big_world": {
 "5000": "a5ee4469310aba2725bdb00017175f7e71f638edd86f6c41eeb7dc1593d32106",
 "5001": "86a5e16e76e3dd6015e7d7aa925917749a8b52e356ff303aa24289221d902838",
 "5002": "eb78f8860ae286559751412ce79de7ff56bc5fedec50f5cde0c005c9f03bedf8",
 "5003": "f9abe0c1561311f7edfdcc82b53c2ea2ea38dc5ce06a0b2634e1975b96aa91c7",
 "5004": "c265bcf8b303dff8027c69cd42c63556679463031f79619c3aa343eab8fdcfe5",
 "5005": "08f741ccbb301a98398a2658b453428cd651457438a4f0b2c01c9d5c43f976a6"
},
 "far_world": {
 "5000": "374b810a35dd456ccd899d5cbb8884223ba6c3a6b5e0a27cda433bb2bc5cb815",
 "5001": "1c4d05ee0d584fcc26fdb27db5b5f5a1a7b4abf61dd64759953f43a9ff51a6bb",
 "5002": "272c9625e326ff574bb400f451fc73afcc096e84ccd8007ea4de71c91701838a",
 "5003": "005f19fb5cb1e1de0a8a97d23c6ece4cf2a3b047bbd2e07122f64172582db173",
 "5004": "2830a64f247f6d71c5f4caf05435bc85de60a9697cffbebb144048283eacc163",
 "5005": "b057d8803344eca296f8d4f8a0fd15d0fa265184ea703b0b1868a7060aeaa893"
},
 "mirror_world": {
 "5000": "f6a798dda43bf9ab4c97602d0881a73b32c3e8f36fd07b6bf014a42293912988",
 "5001": "c4a68653590e8669f6cc04a2774e038393b87ac42e33cdd11e7783cedca92abf",
 "5002": "0cfce21dc959d7dcd34155753324fb260a756406f49197d69692e1eaf75d4f3f",
 "5003": "3baba50069e97acfe0b77d996c6fd7a73541f798d78ade78b714370a2b91078e",
 "5004": "5c437086861cb9c99bd663673ec290c178438f73ce8071290007c381d00848a6",
 "5005": "f021e970b3497fa260244f5b2fb0cc2d96e922edbc763dd0eaa8c5feab06b4f1"
},
 "list_family": {
 "5000": "7a0846c85313cfab6bbafbd78e10635a425ebcad3519d90533cac2d5d816625e",
 "5001": "3a8887f2614e803a963686e221f13870510bdbfe19c7da29f8152ed04fae0355",
 "5002": "7868bdeda541ba2d936df4ec61fffff50eb9a16e61e39e1a2aa2049407efd9c5",
 "5003": "acdf0c84e85cf2f72005dc7c227e921ea852f41534a7ed1b41cc056ac8f82c61",
 "5004": "6786b8835f32257d8c75d33e63383394c6d9502a8b7025b8ceec3d5e59d45747",
 "5005": "aef2ed0d53863ea56cb8d10b6d1e763c201cb53e0e8bc6d23532049d948e6dc9"
}
}
""")


@pytest.mark.parametrize("family", list(A.FAMILIES))
def test_a_seed_still_builds_the_same_world(rtc, family):
    want = DIGESTS[family]
    assert len(want) == (42 if family == "adversarial_scene" else 6)
    for seed, digest in want.items():
        w, cam = A.FAMILIES[family](rtc, int(seed))
        assert A.world_digest(w, cam) == digest, (family, seed)


def _bytes_of_lights(d):
    return {k: bytes(v) for k, v in d.items()}


@pytest.mark.parametrize("name", list(A.GEOMETRIES))
def test_helpers_are_deterministic_finite_and_invertible(rtc, O, name):
    fam, seed = A.GEOMETRIES[name]
    w, cam = A.geometry(rtc, name)
    w2, cam2 = A.FAMILIES[fam](rtc, seed)
    cam2 = A.recamera(rtc, cam2, *A.FRAME)
    assert A.world_digest(w, cam) == A.world_digest(w2, cam2) and (cam.hsize, cam.vsize) == A.FRAME
    big = A.FAMILIES[fam](rtc, seed)[1]
    assert bytes(cam.view_inv) == bytes(big.view_inv) and cam.fov == big.fov           # the same view ...
    assert abs(cam.pixel_size * cam.hsize - big.pixel_size * big.hsize) < 1e-12 or cam.hsize * big.vsize != cam.vsize * big.hsize
    assert A.all_finite(w, cam) and A.passes_determinant_rule(rtc, O, w)
    lights = [A.hostile_lights(rtc, O, w, cam, 3), A.hostile_lights(rtc, O, w2, cam2, 3)]
    assert _bytes_of_lights(lights[0]) == _bytes_of_lights(lights[1]) and tuple(lights[0]) == A.HOSTILE_LIGHTS
    areas = [A.hostile_area_light(rtc, w), A.hostile_area_light(rtc, w2)]
    assert _bytes_of_lights(areas[0]) == _bytes_of_lights(areas[1]) and tuple(areas[0]) == A.HOSTILE_AREA_LIGHTS
    assert A.all_finite(w, cam, list(lights[0].values()) + list(areas[0].values()))
    for a in areas[0].values():
        assert len(A.with_lights(rtc, w, [a]).samples()) == 9
    assert len({A.sample_key(s) for s in A.with_lights(rtc, w, [areas[0]["coincident"]]).samples()}) == 1
    lenses = [A.hostile_lenses(rtc, w, cam), A.hostile_lenses(rtc, w2, cam2)]
    assert list(lenses[0]) == list(lenses[1])
    for k in lenses[0]:
        (spec, c), (spec2, c2) = lenses[0][k], lenses[1][k]
        assert spec == spec2 and bytes(c) == bytes(c2) and A.all_finite(w, c)
        assert np.isfinite(A.lens_origins(rtc, c, spec)).all()
    for refl, refr in A.SHADINGS.values():
        m = A.with_materials(rtc, w, refl, refr)
        assert len(m) == len(w) and bytes(m.light) == bytes(w.light)
        assert all(s.material.transparency == (o.material.transparency if refr else 0.0) for s, o in zip(m.shapes, w.shapes))
        assert all(s.material.reflective == (o.material.reflective if refl else 0.0) for s, o in zip(m.shapes, w.shapes))
        assert all(bytes(s.inv) == bytes(o.inv) and s.kind == o.kind and s.world_id == o.world_id for s, o in zip(m.shapes, w.shapes))
        assert A.passes_determinant_rule(rtc, O, m)
    assert all(s.material.transparency == o.material.transparency for s, o in zip(A.with_materials(rtc, w, True, True).shapes, w.shapes))


def test_the_matrix_geometries_show_lit_shadowed_and_missing_pixels(rtc, O):
    for name in ("one", "two"):
        w, cam = A.geometry(rtc, name)
        c = A.classes(rtc, O, (name, "refr"), w, cam, (A.sample_key(w.light),))
        print(name, len(w), "objects:", c)
        assert c["lit"] > 0 and c["shadowed"] > 0 and c["miss"] > 0, (name, c)
        assert any(s.kind == A.PLANE for s in w.shapes) and A.straddled_sphere(rtc, w, cam) is not None
    assert len(A.geometry(rtc, "one")[0]) <= 256 < len(A.geometry(rtc, "two")[0]) <= 1000


@pytest.mark.parametrize("name", [c.name for c in A.CASES])
def test_every_case_is_of_its_class_and_its_reference_is_not_trivial(rtc, O, name):
    facts = A.check_class(rtc, O, A.BY_NAME[name])
    print(name, facts)


def test_the_case_table_names_every_cell_of_the_matrix():
    """The full product of the axes, computed here: 2 sources x 3 shadings x (3 light forms x 2 cameras - one-light pinhole)
    k_trace cells and 3 sources x 3 light forms k_aov cells; each named by exactly one matrix case."""
    import itertools
    want = {(s, sh, lf, c) for s, sh, lf, c in itertools.product(("cull", "cull2"), ("flat", "refl", "refr"), ("one", "args", "table"), ("pinhole", "lens"))
            if (lf, c) != ("one", "pinhole")}
    want |= {("aov", s, lf) for s, lf in itertools.product(("smem", "cull", "cull2"), ("one", "args", "table"))}
    assert len(want) == 30 + 9
    named = [c.cell for c in A.CASES if c.part in ("matrix", "aov_matrix")]
    assert len(named) == len(set(named)) and set(named) == want == set(A.matrix_cells())
    for c in A.CASES:
        if c.part == "matrix":
            src, sh, lf, camera = c.cell
            assert c.source == A.SOURCES[src][1] and c.shading == sh and c.light_form == lf and bool(c.lens) == (camera == "lens")
            assert c.lens in ("", "straddle_shape") and c.lights == {"one": ("own",), "args": ("own", "near_surface"), "table": ("area", "cross_floor")}[lf]
        if c.part == "aov_matrix":
            assert c.light_form == c.cell[2] and c.source == {"smem": A.SRC_SMEM, "cull": A.SRC_CULL, "cull2": A.SRC_CULL2}[c.cell[1]]
    # the update cases are cells of the matrix, lens + table form, one per culled source
    assert sorted(c.cell for c in A.CASES if c.part == "update") == [("cull", "refr", "table", "lens"), ("cull2", "refr", "table", "lens")]
