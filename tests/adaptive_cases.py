"""Inputs of the adaptive anti-aliasing tests (tests/test_host_adaptive.py, tests/test_gpu_adaptive.py): canvases for the mask,
an independent numpy restatement of the mask, and small Worlds for the composed route."""
import math

import numpy as np

THRESHOLDS = (-1.0, 0.0, 0.01, 0.25, math.inf)
SIZES = ((1, 1), (1, 7), (7, 1), (2, 2), (33, 9), (37, 19), (70, 40))   # (width, height)
TILE_SIZES = ((31, 7), (32, 8), (33, 9), (64, 16), (65, 17))            # around the 32 x 8 tile of k_aa_mask
CANVAS_NAMES = ([f"random-{w}x{h}" for w, h in SIZES] + [f"quarters-{w}x{h}" for w, h in SIZES[3:]] +
                ["constant-37x19", "constant-1x1", "special-37x19", "special-7x1"])
TILE_NAMES = [f"random-{w}x{h}" for w, h in TILE_SIZES] + [f"quarters-{w}x{h}" for w, h in TILE_SIZES[2:]] + ["special-65x17"]


def canvas(name):
    """The (H, W, 3) f64 canvas of a case: `random` = flat patches of a few pixels with noise of a few thousandths on top, so that
    every threshold splits the pixels; `quarters` = every channel a multiple of 1/4, so that distances land exactly on 0.25 and on
    0; `constant`; `special` = a random canvas with NaN, +inf, -inf and -0.0 sprinkled in."""
    kind, size = name.split("-")
    w, h = (int(v) for v in size.split("x"))
    rng = np.random.default_rng(1000 * w + h + len(kind))
    if kind == "constant":
        return np.full((h, w, 3), 0.375)
    if kind == "quarters":
        return rng.integers(0, 3, size=(h, w, 3)).astype(np.float64) * 0.25
    patches = rng.integers(0, 4, size=((h + 2) // 3, (w + 3) // 4, 3)).astype(np.float64) * 0.25
    rgb = np.repeat(np.repeat(patches, 3, axis=0), 4, axis=1)[:h, :w] + rng.uniform(0.0, 0.008, size=(h, w, 3))
    if kind == "special":
        flat = rgb.reshape(-1)
        for k, v in enumerate((math.nan, math.inf, -math.inf, -0.0, 0.0)):
            flat[rng.choice(flat.size, size=max(1, flat.size // 40), replace=False)] = v
    return np.ascontiguousarray(rgb)


def mask_restated(rgb, mode, threshold):
    """The statement of include/rtc.h in numpy: an edge between two horizontally or vertically adjacent pixels of the rendered area
    flags both when its distance sqrt(((dr*dr) + (dg*dg)) + (db*db)) is > threshold (NaN compares false)."""
    h, w = rgb.shape[:2]
    rw, rh = (w - 1, h - 1) if mode == 0 else (w, h)
    mask = np.zeros((h, w), dtype=np.uint8)
    if rw <= 0 or rh <= 0:
        return mask
    r = rgb[:rh, :rw]

    def far(a, b):
        with np.errstate(invalid="ignore", over="ignore"):
            d = a - b
            return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) > threshold

    horiz = far(r[:, :-1], r[:, 1:])   # edge (x, x+1)
    vert = far(r[:-1, :], r[1:, :])    # edge (y, y+1)
    m = mask[:rh, :rw]
    m[:, :-1] |= horiz
    m[:, 1:] |= horiz
    m[:-1, :] |= vert
    m[1:, :] |= vert
    return mask


# ---- Worlds of the composed route --------------------------------------------------------------------------------------------
WORLDS = ("trio", "grid290", "two-lights", "area9", "updated")
ORACLE_WORLDS = ("trio", "grid290", "updated")   # one point light: the CPU oracle renders them
FRAME_SIZES = ((37, 19), (96, 54))
SPECS = ((2, 2), (4, 4), (3, 5))
TINY = (9, 5)                                    # the frame of the 16 x 16 spec and of the one-pixel chunks


def trio_shapes(rtc, shift=0.0):
    """A checkered floor, a mirror ball and a glass ball; `shift` moves the balls (the World before its update)."""
    M = rtc.Matrix
    floor = rtc.material(specular=0.0, reflective=0.2, pattern=("checker", (0.85, 0.85, 0.8), (0.2, 0.2, 0.3), None))
    mirror = rtc.material(color=(0.9, 0.5, 0.4), diffuse=0.5, specular=0.8, reflective=0.6)
    glass = rtc.material(color=(0.05, 0.1, 0.05), ambient=0.0, diffuse=0.3, specular=0.9, shininess=300.0, reflective=0.9, transparency=0.9,
                         refractive_index=1.5)
    return [rtc.plane(M.identity(), floor), rtc.sphere(M.identity().translation(-1.2 + shift, 1.0, 0.5), mirror),
            rtc.sphere(M.identity().scaling(0.7, 0.7, 0.7).translation(0.9 + shift, 0.7, -0.8), glass)]


def camera(rtc, name, width, height):
    """Level cameras: the upper part of every frame is empty sky, which no threshold above 0 flags."""
    M = rtc.Matrix
    if name == "grid290":
        return rtc.camera(width, height, 0.9, M.make_view_transform((0.5, 1.6, -11.0), (0.0, 1.9, 0.0), (0.0, 1.0, 0.0)))
    return rtc.camera(width, height, 0.9, M.make_view_transform((0.0, 1.2, -6.0), (0.0, 1.7, 0.0), (0.0, 1.0, 0.0)))


def world(rtc, name, before_update=False):
    """The host World `name`. "updated" is the trio with its balls moved: the DeviceWorld is created from
    world(rtc, "updated", before_update=True), which has one shape more, and then updated to this one."""
    M = rtc.Matrix
    if name in ("trio", "updated"):
        w = rtc.World(rtc.light((-6.0, 8.0, -8.0)))
        for s in trio_shapes(rtc, 0.0 if name == "trio" else (0.6 if before_update else 0.25)):
            w.add_shape(s)
        if before_update:
            w.add_shape(rtc.cube(M.identity().translation(0.0, 1.0, 3.0), rtc.material(color=(0.2, 0.9, 0.3))))
        return w
    if name == "two-lights":
        w = rtc.World([rtc.light((-6.0, 8.0, -8.0)), rtc.light((7.0, 5.0, -3.0), (0.5, 0.5, 0.6))])
    elif name == "area9":
        w = rtc.World([rtc.area_light((-3.0, 7.0, -7.0), (3.0, 0.0, 0.0), (0.0, 0.0, 3.0), 3, 3)])
    elif name == "grid290":
        w = rtc.World(rtc.light((-10.0, 10.0, -10.0)))
        w.add_shape(rtc.plane(M.identity(), rtc.material(specular=0.0, pattern=("checker", (0.8, 0.8, 0.8), (0.3, 0.3, 0.35), None))))
        colours = ((0.9, 0.15, 0.1), (0.1, 0.8, 0.2), (0.15, 0.2, 0.9))
        for i in range(17):
            for j in range(17):
                mat = rtc.material(color=colours[(i * 17 + j) % 3], specular=0.4, reflective=0.3 if (i * 17 + j) % 5 == 0 else 0.0)
                x, z = i - 8.0, j - 8.0
                if (i + j) % 2:
                    w.add_shape(rtc.sphere(M.identity().scaling(0.45, 0.45, 0.45).translation(x, 0.45, z), mat))
                else:
                    w.add_shape(rtc.cube(M.identity().scaling(0.4, 0.35, 0.4).translation(x, 0.35, z), mat))
        return w
    else:
        raise KeyError(name)
    for s in trio_shapes(rtc):
        w.add_shape(s)
    return w


def expected_launches(pixels_refined, n, max_rays):
    per = (max_rays if max_rays else 1 << 21) // n
    return -(-pixels_refined // per)
