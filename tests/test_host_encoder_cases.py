"""The writers' boundary cases (encoder_cases.py) on the host statement: every case's predicate holds, so each case provably
reaches its branch; each file decodes to the expected pixels with the suites' independent decoders; the numpy median cut
equals the host quantiser on frames beyond the cases. CPU only."""
import io
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import encoder_cases as E  # noqa: E402
import test_host_gif as HG  # noqa: E402
import test_host_jpeg as HJ  # noqa: E402
import test_host_png as HP  # noqa: E402

CASES = E.all_cases()
IDS = [c.name for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_predicate_on_host_statement(case):
    px = case.pixels()
    if case.kind == "packed":
        for fmt in case.formats:
            case.check(px, case.host(fmt), fmt)
    else:
        case.check(px, case.host())


@pytest.mark.parametrize("case", [c for c in CASES if c.kind != "packed"], ids=[c.name for c in CASES if c.kind != "packed"])
def test_host_file_decodes(case):
    from PIL import Image
    px, b = case.pixels(), case.host()
    if case.kind == "png":
        got, _, _ = HP.decode(b)     # zlib and the own unfilterer
        assert np.array_equal(got, px)
        _, out = HP.inflate_blocks(b"".join(d for t, d in HP.chunks(b) if t == b"IDAT"))   # the own inflater
        assert out == E.rtc.png_filter(px)[1].tobytes()
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(b))), px)
    elif case.kind == "jpeg":
        im = np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))
        assert im.shape == px.shape
        if case.quality == 100 and px.size <= 1 << 16:
            assert np.array_equal(HJ.decode_coefficients(b), E.rtc.jpeg_coefficients(px, 100))
    else:
        g = HG.parse_gif(b)          # the own parser and LZW decoder
        pal, idx, _ = E.rtc.gif_quantize(px)
        assert np.array_equal(HG.decoded_rgb(g)[0], pal[idx])
        pil = HG.pil_frames(b)
        assert len(pil) == 1 and np.array_equal(pil[0], pal[idx])


def test_every_case_is_listed_in_the_module_docstring():
    doc = E.__doc__
    for c in CASES:
        assert c.name in doc or c.name.rsplit("_", 1)[0] + "_*" in doc or c.name.startswith(("packed_len_", "packed_w")), c.name
    assert len(set(IDS)) == len(IDS)
    assert {"png_encode", "PngEncoder", "image:png"} <= {e for c in CASES for e in c.entries}


def test_numpy_median_cut_equals_the_host_quantiser():
    """The numpy statement of the cut against rtc_gif_quantize on frames the cases do not build: rendered canvases, noise,
    gradients and the host suite's own small median-cut frame."""
    rng = np.random.default_rng(5)
    frames = [HG.gradient(64, 80), HG.gradient(7, 300), rng.integers(0, 256, (40, 50, 3), dtype=np.uint8),
              (rng.integers(0, 8, (30, 40, 3)) * 32 + rng.integers(0, 3, (30, 40, 3))).astype(np.uint8), HG.small_median_cut_frame()]
    for name in ("jamis_100x50", "synthetic100_96x54", "test7_80x60"):
        canvas = np.load(HG.ROOT / "tests" / "golden" / f"{name}.npy")
        frames.append(np.ascontiguousarray(E.rtc.to_rgba8(canvas)[..., :3]))
    for f in frames:
        pal, idx, used = E.rtc.gif_quantize(f)
        npal, nused, _ = E.median_cut_np(f)
        assert nused == used and np.array_equal(npal, pal)
        assert np.array_equal(idx.ravel(), HG.brute_nearest(f, npal))


def test_lzw_trace_agrees_with_the_host_stream():
    """lzw_trace's restarts are the clear codes rtc_gif_lzw writes inside one segment."""
    rng = np.random.default_rng(9)
    for n in (100, 3000, HG.S):
        idx = rng.integers(0, 256, n).astype(np.uint8)
        _, restarts, _ = E.lzw_trace(idx)
        assert HG.n_clears(E.rtc.gif_lzw(idx)) == 1 + len(restarts)
