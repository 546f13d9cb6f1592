"""Sequential numpy / Python restatement of the component outlines (sc_component_outlines / starcop_amd.plumes.component_outlines),
its invariant checks and the masks the outline tests share.

The outline of component k of a label image: one directed unit edge on the lattice of pixel corners for every side of a pixel of
value k whose neighbour is not k (or outside), with k on the right of the direction of travel (row axis down).  Directions:
0 east (a top side), 1 south (a right side), 2 west (a bottom side), 3 north (a left side).  Edges are numbered in raster order
of their pixel, then top, right, bottom, left.  The successor of an edge leaves its end corner and has the same value; where there
are two candidates, connectivity 2 takes the left turn and connectivity 1 the right turn.
"""
import numpy as np
import scipy.ndimage as ndi

STEP = ((0, 1), (1, 0), (0, -1), (-1, 0))                      # (d row, d col) of the four directions
START = ((0, 0), (0, 1), (1, 1), (1, 0))                       # start corner of side d, relative to the pixel

# seeds of the Bernoulli masks, one per (p, connectivity) case and one for the large image
SEEDS = {0.3: 301, 0.5: 502, 0.62: 623, 0.8: 804}
SEED_LARGE = 130258
SEED_BATCH = (71, 72)


def label(mask, connectivity):
    """scipy.ndimage.label with the structure of the connectivity -> (int32 labels, count)"""
    lab, n = ndi.label(mask, structure=np.ones((3, 3)) if connectivity == 2 else None)
    return lab.astype(np.int32), int(n)


def edge_list(lab):
    """-> list of (start row, start col, direction, value) in edge order"""
    H, W = lab.shape
    P = np.pad(lab, 1)
    out = []
    for r in range(H):
        for c in range(W):
            k = int(lab[r, c])
            if k <= 0:
                continue
            across = (P[r, c + 1], P[r + 1, c + 2], P[r + 2, c + 1], P[r + 1, c])      # above, right, below, left
            for d in range(4):
                if across[d] != k:
                    out.append((r + START[d][0], c + START[d][1], d, k))
    return out


def successors(edges, connectivity):
    index = {e: i for i, e in enumerate(edges)}
    succ = np.empty(len(edges), dtype=np.int64)
    for i, (r, c, d, k) in enumerate(edges):
        er, ec = r + STEP[d][0], c + STEP[d][1]
        left, right = (d + 3) % 4, (d + 1) % 4
        for nd in ((left, d, right) if connectivity == 2 else (right, d, left)):
            j = index.get((er, ec, nd, k))
            if j is not None:
                succ[i] = j
                break
        else:
            raise AssertionError("an outline that does not continue")
    return succ


def walk(succ):
    """-> the rings as lists of edge ids, each from its smallest edge on, in order of that edge"""
    seen = np.zeros(len(succ), dtype=bool)
    rings = []
    for i in range(len(succ)):
        if seen[i]:
            continue
        ring, j = [], i
        while not seen[j]:
            seen[j] = True
            ring.append(j)
            j = int(succ[j])
        assert j == i, "the successors do not form cycles"
        rings.append(ring)
    return rings


def outlines_ref(lab, connectivity, collinear=False):
    """the four arrays of component_outlines, plus ``n_edges`` and ``longest`` (edges of the longest ring)"""
    edges = edge_list(lab)
    rings = walk(successors(edges, connectivity)) if edges else []
    recs = []
    for ring in rings:
        v = np.array([(edges[j][0], edges[j][1]) for j in ring], dtype=np.int64)          # (row, col)
        d = np.array([edges[j][2] for j in ring])
        nxt = np.roll(v, -1, axis=0)
        a2 = int(np.sum(v[:, 1] * nxt[:, 0] - nxt[:, 1] * v[:, 0]))
        if not collinear:
            v = v[np.roll(d, 1) != d]                           # incoming direction != outgoing; order from the smallest edge stays
        recs.append((edges[ring[0]][3], 0 if a2 > 0 else 1, ring[0], v, a2))
    recs.sort(key=lambda t: t[:3])
    lens = [len(t[3]) for t in recs]
    return {"vertices": (np.concatenate([t[3] for t in recs]) if recs else np.zeros((0, 2))).astype(np.int32).reshape(-1, 2),
            "ring_offsets": np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
            "ring_label": np.array([t[0] for t in recs], dtype=np.int32),
            "ring_area2": np.array([t[4] for t in recs], dtype=np.int64),
            "n_edges": len(edges), "longest": max((len(r) for r in rings), default=0)}


def even_odd_fill(ring, H, W):
    """pixels whose centre an even-odd ray to the left crosses an odd number of times: ring is an open (n, 2) array of (row, col)
    corners joined by axis-parallel segments -> bool (H, W)"""
    D = np.zeros((H, W + 1), dtype=np.int64)
    nxt = np.roll(ring, -1, axis=0)
    for (r0, c0), (r1, c1) in zip(ring.tolist(), nxt.tolist()):
        assert (r0 == r1) != (c0 == c1), "a segment that is not axis-parallel or is empty"
        if c0 == c1:
            D[min(r0, r1):max(r0, r1), c0] += 1
    return (np.cumsum(D, axis=1)[:, :W] % 2).astype(bool)


def check_invariants(lab, count, out):
    """one exterior per component, half the sum of the doubled areas = the pixel count, the even-odd fill of the rings = the pixels"""
    H, W = lab.shape
    off, rl, a2 = out["ring_offsets"], out["ring_label"], out["ring_area2"]
    assert sorted(set(rl.tolist())) == list(range(1, count + 1))
    assert np.all(a2 != 0)
    for k in range(1, count + 1):
        idx = np.nonzero(rl == k)[0]
        assert (a2[idx] > 0).sum() == 1 and a2[idx[0]] > 0, f"component {k}: not exactly one exterior, or not first"
        assert a2[idx].sum() == 2 * int((lab == k).sum())
        fill = np.zeros((H, W), dtype=bool)
        for q in idx:
            fill ^= even_odd_fill(out["vertices"][off[q]:off[q + 1]].astype(np.int64), H, W)
        assert np.array_equal(fill, lab == k), f"component {k}: the fill of its rings is not the component"
    keys = list(zip(rl.tolist(), (a2 < 0).tolist()))
    assert keys == sorted(keys)


def spiral(n=33):
    """a one-pixel-wide square spiral on n x n"""
    g = np.zeros((n, n), dtype=bool)
    r0, c0, r1, c1 = 0, 0, n - 1, n - 1
    while r0 <= r1 and c0 <= c1:
        g[r0, c0:c1 + 1] = 1
        g[r0:r1 + 1, c1] = 1
        g[r1, c0:c1 + 1] = 1
        g[r0 + 2:r1 + 1, c0] = 1
        if c0 + 1 <= c1:
            g[r0 + 2, c0:c0 + 2] = 1
        r0 += 2; c0 += 2; r1 -= 2; c1 -= 2
    return g


def bernoulli(shape, p, seed):
    return np.random.default_rng(seed).random(shape) < p


def hand_masks():
    """name -> bool mask, at most 16 x 16"""
    m = {}
    m["empty"] = np.zeros((5, 7), dtype=bool)
    m["full"] = np.ones((6, 9), dtype=bool)
    one = np.zeros((5, 6), dtype=bool); one[2, 3] = 1
    m["one_pixel"] = one
    dg = np.zeros((4, 5), dtype=bool); dg[1, 1] = dg[2, 2] = 1
    m["diagonal_pair"] = dg
    sq = np.zeros((9, 10), dtype=bool); sq[1:8, 2:9] = 1; sq[3:6, 4:7] = 0
    m["square_ring"] = sq
    pinch = np.zeros((10, 11), dtype=bool); pinch[1:9, 1:10] = 1; pinch[3:5, 3:5] = 0; pinch[5:7, 5:7] = 0
    m["pinched_hole"] = pinch                                   # the two background squares meet diagonally at corner (5, 5)
    isl = np.zeros((13, 14), dtype=bool); isl[1:12, 1:13] = 1; isl[3:10, 3:11] = 0; isl[5:8, 5:9] = 1
    m["island_in_hole"] = isl
    m["checkerboard"] = (np.indices((8, 8)).sum(0) % 2) == 0
    return m


def all_small_masks():
    """the hand-made masks, the spiral and the four Bernoulli masks: name -> mask"""
    m = hand_masks()
    m["spiral"] = spiral()
    for p, seed in SEEDS.items():
        m[f"bernoulli_{p}"] = bernoulli((37, 70), p, seed)
    return m
