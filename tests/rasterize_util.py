"""numpy float64 restatement of the polygon burn (sc_rasterize_polygons / starcop_amd.plumes.rasterize_polygons) and the polygons
the rasterize tests share.

The rule, as include/starcop_hip.h states it: rings in pixel coordinates (col, row), pixel (r, c) has its centre at
(c + 0.5, r + 0.5); an edge (x0, y0) -> (x1, y1) crosses the scanline yc = r + 0.5 iff (y0 <= yc) != (y1 <= yc); the crossing
abscissa is xs = x0 + ((yc - y0) * (x1 - x0)) / (y1 - y0), every operation a numpy ufunc of its own (numpy does not fuse across
ufuncs); the crossing toggles pixel c iff xs <= c + 0.5; a pixel is covered when the toggles of all rings of the polygon are odd;
polygons burn in order, the later one wins.
"""
import functools

import numpy as np

import outlines_util as OU

GT = (500000.0, 5.0, 0.0, 3600000.0, 0.0, -5.0)
SEED_GENERAL = 20261
SHAPES_GENERAL = ((64, 96), (61, 67))


def ring_edges(rings):
    """all rings of a polygon, each closed -> x0, y0, x1, y1"""
    parts = []
    for ring in rings:
        a = np.asarray(ring, dtype=np.float64)
        if (a[0] != a[-1]).any():
            a = np.concatenate([a, a[:1]])
        parts.append(np.concatenate([a[:-1], a[1:]], 1))
    e = np.concatenate(parts)
    return e[:, 0], e[:, 1], e[:, 2], e[:, 3]


def raster_ref(polys, values, H, W):
    """polys: list of ring lists in pixel coordinates (None burns nothing); values: what each burns -> int32 (H, W)"""
    out = np.zeros((H, W), dtype=np.int32)
    centres = np.arange(W, dtype=np.float64) + 0.5
    for rings, v in zip(polys, values):
        if rings is None:
            continue
        x0, y0, x1, y1 = ring_edges(rings)
        cover = np.zeros((H, W), dtype=bool)
        # rows outside [min y - 1, max y + 1] have no crossing: skipped for time only
        lo = max(int(np.floor(min(y0.min(), y1.min()))) - 1, 0)
        hi = min(int(np.ceil(max(y0.max(), y1.max()))) + 1, H)
        for r in range(lo, hi):
            yc = r + 0.5
            cross = (y0 <= yc) != (y1 <= yc)
            if not cross.any():
                continue
            a0, b0, a1, b1 = x0[cross], y0[cross], x1[cross], y1[cross]
            t = yc - b0
            dx = a1 - a0
            m = t * dx
            dy = b1 - b0
            q = m / dy
            xs = a0 + q
            cover[r] = ((xs[:, None] <= centres[None, :]).sum(0) & 1).astype(bool)
        out[cover] = v
    return out


def to_pixel(rings, gt):
    return [np.stack([(np.asarray(r)[:, 0] - gt[0]) / gt[1], (np.asarray(r)[:, 1] - gt[3]) / gt[5]], 1) for r in rings]


def same_rings(a, b):
    """two closed rings with the same vertex cycle, whatever their start and winding"""
    a, b = np.asarray(a)[:-1], np.asarray(b)[:-1]
    if a.shape != b.shape:
        return False
    for cand in (b, b[::-1]):
        for s in range(len(cand)):
            if np.array_equal(a, np.roll(cand, s, axis=0)):
                return True
    return False


# ---- the polygons of the general test (test 2), seeded ----

def _star(rng, H, W, n):
    cx, cy = rng.uniform(0, W), rng.uniform(0, H)
    ang = np.sort(rng.uniform(0, 2 * np.pi, 2 * n))
    rad = np.where(np.arange(2 * n) % 2 == 0, rng.uniform(6, 25), rng.uniform(1, 6)) * rng.uniform(0.7, 1.3, 2 * n)
    return np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1)


def tie_polygons():
    """the tie cases on any raster of at least 30 x 50: name -> ring list"""
    return {
        "half_integer_square": [np.array([(2.5, 2.5), (6.5, 2.5), (6.5, 6.5), (2.5, 6.5)])],
        # vertices on scanlines (y = 3.5, 7.5, 11.5), and with slope 1 every crossing falls exactly on a centre
        "diamond_on_centres": [np.array([(10.5, 3.5), (14.5, 7.5), (10.5, 11.5), (6.5, 7.5)])],
        # a spike whose tip touches a scanline from below and one from above: local extrema on the scanline
        "tips_on_scanline": [np.array([(20.0, 9.0), (22.25, 4.5), (24.5, 9.0), (26.75, 13.5), (29.0, 9.0), (29.0, 16.0), (20.0, 16.0)])],
        "horizontal_on_scanline": [np.array([(30.2, 20.5), (40.7, 20.5), (40.7, 25.5), (30.2, 25.5)])],
        "crossing_on_centre": [np.array([(41.0, 2.0), (46.0, 7.0), (41.0, 12.0)])],          # xs = 43.5 exactly at yc = 4.5
        "closed_ring_with_hole": [np.array([(3.0, 14.0), (18.0, 14.0), (18.0, 28.0), (3.0, 28.0), (3.0, 14.0)]),
                                  np.array([(6.5, 17.5), (6.5, 24.5), (14.5, 24.5), (14.5, 17.5)])],
    }


@functools.lru_cache(maxsize=None)
def general_polygons(shape):
    """the seeded set on a raster: list of ring lists in pixel coordinates, overlapping freely"""
    H, W = shape
    rng = np.random.default_rng(SEED_GENERAL + H * 1000 + W)
    polys = []
    for n in (3, 5, 8):                                                    # stars
        polys.append([_star(rng, H, W, n)])
    for n in (5, 7, 9):                                                    # vertices in random order: self-intersecting
        polys.append([np.stack([rng.uniform(-5, W + 5, n), rng.uniform(-5, H + 5, n)], 1)])
    for _ in range(3):                                                     # vertices far outside the raster
        far = np.stack([rng.uniform(-1e6, 1e6, 3), rng.uniform(-1e6, 1e6, 3)], 1)
        far[0] = (rng.uniform(0, W), rng.uniform(0, H))
        polys.append([far])
    for _ in range(4):                                                     # slivers thinner than a pixel
        p, d = np.array([rng.uniform(0, W), rng.uniform(0, H)]), rng.uniform(-1, 1, 2)
        d /= np.hypot(*d)
        nrm, L, w = np.array([-d[1], d[0]]), rng.uniform(10, 60), rng.uniform(0.05, 0.6)
        polys.append([np.stack([p, p + L * d, p + L * d + w * nrm, p + w * nrm])])
    polys.append([_star(rng, H, W, 6), _star(rng, H, W, 4)])                # two rings, even-odd where they overlap
    polys.extend(tie_polygons().values())
    return polys


@functools.lru_cache(maxsize=None)
def general_ref(shape):
    polys = general_polygons(shape)
    ref = raster_ref(polys, range(1, len(polys) + 1), *shape)
    ref.setflags(write=False)
    return ref


def comb(teeth=1000, W=4100, H=8):
    """one polygon of `teeth` teeth across the raster: a base along rows 5..6, teeth up to row 1 -> every row 1..4 has
    2 * teeth crossings"""
    pitch = (W - 4.3) / teeth
    pts = [(2.1, 6.6), (2.1, 5.2)]
    for k in range(teeth):
        a = 2.1 + k * pitch
        pts += [(a + 0.2 * pitch, 5.2), (a + 0.35 * pitch, 0.8), (a + 0.65 * pitch, 0.8), (a + 0.8 * pitch, 5.2)]
    pts += [(2.1 + teeth * pitch, 5.2), (2.1 + teeth * pitch, 6.6)]
    return [np.array(pts)]


def bernoulli_cases():
    """(name, mask): the masks of the outline tests and the 37 x 53 Bernoulli masks"""
    cases = sorted(OU.all_small_masks().items())
    cases += [(f"bernoulli53_{p}", OU.bernoulli((37, 53), p, seed)) for p, seed in OU.SEEDS.items()]
    return cases
