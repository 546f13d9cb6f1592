"""Every launch form of sc_mag1c_groups against oracle/mag1c_ref in float64, at the band-count and pixel-count edges of the kernels.

sc_mag1c_variant (a pure host function, the rule sc_mag1c_groups switches on) names the launch or pair of launches a call takes.
Every case below first asserts the code it is meant to reach and then compares mf and albedo ON EVERY PIXEL with the oracle
evaluated in float64 on the same radiances -- never with a float32 evaluation of the oracle: at 112 bands and more with S + 30
pixels that evaluation's own rounding noise exceeds the suite's 0.2 % allowance.  Tolerances are the project's (test_gpu_mag1c.py):
float32 radiances mf 1e-5 of max(|ref|, 1), float64 radiances 1e-6, albedo 1e-6; compute_energy 2e-6 for the rmf scalar and 2e-5
for the per-iteration terms.

Data: the generator of test_paired_launch_mixed_group_sizes (per-band base, 5 % noise, a common brightness term, enhancement on
every 7th pixel, template -|N(0,1)| * 0.3); groups keep P >= S + 30 (well posed), except the single band with 11 pixels.  Each case
asserts that some mf > 0, and runs behind a launch that leaves NaN in the LDS of every CU (nan_in_lds): a kernel that reads LDS it
has not written shows (that is how k_mag1c<double, NT, true> was found to take 0 * tau of an unwritten tau into the rmf energy).  tests/test_mag1c_variants_host.py checks (without a GPU) that the tables reach every code the rule can
return, each with a plain case (S a multiple of 16, P a multiple of 512) and a ragged one (S = 1 mod 16, P no multiple of 16)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mag1c_ref  # noqa: E402
from starcop_amd import _lib  # noqa: E402
from starcop_amd import mag1c as hip_mag1c  # noqa: E402

DEV = "cuda"
L = _lib.MAG1C_LAUNCHES                       # name -> code of enum sc_mag1c_launch
TOL_MF = {"f32": 1e-5, "f64": 1e-6}
TOL_ALB = 1e-6
NP_DT = {"f32": np.float32, "f64": np.float64}
UNTOUCHED = -7                                # what status[] is filled with before a direct call of the C ABI
WORST = {}                                    # code -> worst relative error of mf seen by the tests of this module


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / max(float(np.abs(b).max()), 1.0)


def variant(S, dt, alpha, energy=False, direct=False):
    return _lib.load().sc_mag1c_variant(int(S), int(dt == "f64"), int(alpha == 0.0), int(energy), int(direct))


def note(code, err):
    WORST[code] = max(WORST.get(code, 0.0), float(err))


def radiances(S, n, seed):
    """(n, S) float64 radiances and the template, as test_paired_launch_mixed_group_sizes makes them"""
    rng = np.random.default_rng(seed)
    t = -np.abs(rng.standard_normal(S)) * 0.3
    base = rng.uniform(1, 6, size=S)
    x = base * (1 + 0.05 * rng.standard_normal((n, S))) + 0.2 * rng.standard_normal((n, 1)) * base
    conc = np.zeros(n); conc[::7] = 1500.0
    return x * (1 + conc[:, None] * 1e-5 * t), t


class launches:
    """records the variant code of every sc_mag1c_groups call made through the Python wrappers while it is active"""

    def __enter__(self):
        lib = _lib.load()
        self.lib, self.orig, self.codes = lib, lib.sc_mag1c_groups, []

        def spy(aref, st):
            a = aref._obj
            self.codes.append(lib.sc_mag1c_variant(a.S, a.x_is_f64, int(a.alpha == 0.0), int(bool(a.energy)), int(bool(a.cube))))
            return self.orig(aref, st)
        lib.sc_mag1c_groups = spy
        return self

    def __exit__(self, *exc):
        self.lib.sc_mag1c_groups = self.orig


# ------------------------------------------------------------------------------------------------ groups of one launch (C ABI)
# (code, S, element type, alpha, pixels per group in launch order; 0: a skipped group)
def _mixed(S):
    return (1025, 511, S + 30, 0, 1537, 512, 1024, 513)


GROUP_CASES = [
    # fp32, alpha = 0, up to 64 bands: k_mag1c_tile<4, false, false>
    ("TILE4", 64, "f32", 0.0, (1024, 0, 512)),
    ("TILE4", 17, "f32", 0.0, (513, 47, 0, 1025, 511)),
    ("TILE4", 1, "f32", 0.0, (31, 0, 11)),
    ("TILE4", 15, "f32", 0.0, (45, 0, 513)),
    ("TILE4", 16, "f32", 0.0, (512, 46, 0, 1537)),
    ("TILE4", 48, "f32", 0.0, (78, 0, 1025)),
    ("TILE4", 64, "f32", 0.0, (94, 0, 1025, 511)),
    # fp32, alpha != 0: k_mag1c_tile<4, false, true>
    ("TILE4_SHRINK", 64, "f32", 1e-4, (512, 0, 1024)),
    ("TILE4_SHRINK", 17, "f32", 1e-4, (1025, 0, 47, 513)),
    ("TILE4_SHRINK", 1, "f32", 1e-4, (31, 0, 11)),
    ("TILE4_SHRINK", 16, "f32", 1e-4, (46, 0, 511)),
    ("TILE4_SHRINK", 48, "f32", 1e-4, (1024, 0, 78)),
    ("TILE4_SHRINK", 64, "f32", 1e-4, (513, 0, 94)),
    # fp32, more than 64 bands: the resident + streaming pair, every group taken by exactly one of the two
    ("TILE8_PAIR", 80, "f32", 0.0, (1024, 0, 512)),
    ("TILE8_PAIR", 65, "f32", 0.0, _mixed(65)),
    ("TILE8_PAIR", 128, "f32", 0.0, _mixed(128)),
    ("TILE8_PAIR", 112, "f32", 0.0, (142, 0, 513)),
    ("TILE8_PAIR", 113, "f32", 0.0, (600, 0, 143)),
    ("TILE8_PAIR_SHRINK", 128, "f32", 1e-4, (512, 0, 1024)),
    ("TILE8_PAIR_SHRINK", 65, "f32", 1e-4, (1025, 511, 0, 95, 513)),
    ("TILE8_PAIR_SHRINK", 113, "f32", 1e-4, (143, 0, 1537)),
    ("TILE8_PAIR_SHRINK", 80, "f32", 1e-4, (110, 0, 1024)),
    ("TILE8_PAIR_SHRINK", 112, "f32", 1e-4, (512, 0, 142)),
    ("TILE8_PAIR_SHRINK", 128, "f32", 1e-4, (158, 0, 1025)),
    # fp64, alpha = 0: k_mag1c_fast<double, 1024> for every band count
    ("F64_FAST", 128, "f64", 0.0, (512, 0, 1024)),
    ("F64_FAST", 65, "f64", 0.0, (1025, 0, 95, 513)),
    ("F64_FAST", 1, "f64", 0.0, (41, 0, 11)),
    ("F64_FAST", 16, "f64", 0.0, (46, 0, 511)),
    ("F64_FAST", 17, "f64", 0.0, (1025, 0, 47)),
    ("F64_FAST", 64, "f64", 0.0, (94, 0, 1025)),
    ("F64_FAST", 113, "f64", 0.0, (143, 0, 600)),
    # fp64, alpha != 0, up to 64 bands: k_mag1c<double, 512>
    ("F64_512", 64, "f64", 1e-4, (512, 0, 1024)),
    ("F64_512", 17, "f64", 1e-4, (47, 0, 1025)),
    ("F64_512", 1, "f64", 1e-4, (41, 0, 11)),
    ("F64_512", 15, "f64", 1e-4, (45, 0, 513)),
    ("F64_512", 16, "f64", 1e-4, (511, 0, 46)),
    ("F64_512", 48, "f64", 1e-4, (78, 0, 600)),
    ("F64_512", 64, "f64", 1e-4, (1025, 0, 94)),
    # fp64, alpha != 0, more than 64 bands: k_mag1c<double, 1024>
    ("F64_1024", 128, "f64", 1e-4, (1024, 0, 512)),
    ("F64_1024", 65, "f64", 1e-4, (1025, 0, 95)),
    ("F64_1024", 128, "f64", 1e-4, (158, 0, 1025)),
    ("F64_1024", 80, "f64", 1e-4, (110, 0, 513)),
    ("F64_1024", 112, "f64", 1e-4, (142, 0, 511)),
    ("F64_1024", 113, "f64", 1e-4, (1537, 0, 143)),
]


def group_id(c):
    return f"{c[0]}-S{c[1]}-{c[2]}-P" + "_".join(str(p) for p in c[4])


def run_packed(x, sizes, t, num_iter=30, alpha=0.0, k=1.0, flags=(0, 0, 0, 1)):
    """sc_mag1c_pack + sc_mag1c_groups through the C ABI on groups of consecutive rows of x ((n, S) float32 | float64; the rows are
    handed over in a shuffled cube and found again through pix_index).  Outputs NaN-filled with 64 elements behind them, status
    filled with UNTOUCHED.  -> (mf [n], albedo [n], status [G]) numpy"""
    lib = _lib.load()
    n, S = x.shape
    assert n == sum(sizes)
    is64 = int(x.dtype == np.float64)
    perm = np.random.default_rng(n + S).permutation(n)
    cube_np = np.empty_like(x); cube_np[perm] = x
    cube = torch.from_numpy(cube_np).to(DEV)
    pix = torch.from_numpy(perm.astype(np.int64)).to(DEV)
    counts = torch.as_tensor(sizes, dtype=torch.int64)
    G = int(counts.numel())
    ppad = ((counts + 63) // 64) * 64
    poff = torch.cumsum(counts, 0) - counts
    xoff = torch.cumsum(ppad * S, 0) - ppad * S
    xp = torch.full((int((ppad * S).sum()),), float("nan"), dtype=cube.dtype, device=DEV)      # sc_mag1c_pack writes the padding too
    P_d, ppad_d = counts.to(torch.int32).to(DEV), ppad.to(torch.int32).to(DEV)
    poff_d, xoff_d = poff.to(DEV), xoff.to(DEV)
    st = _lib.stream()
    _lib.check(lib.sc_mag1c_pack(_lib.ptr(cube), is64, S, 0, S, _lib.ptr(pix), _lib.ptr(xoff_d), _lib.ptr(ppad_d), _lib.ptr(poff_d),
                                 _lib.ptr(P_d), G, _lib.ptr(xp), is64, st))
    assert not bool(torch.isnan(xp).any())
    templ = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64)).to(DEV)
    mf = torch.full((n + 64,), float("nan"), dtype=cube.dtype, device=DEV)
    alb = torch.full((n + 64,), float("nan"), dtype=cube.dtype, device=DEV)
    work = torch.zeros(lib.sc_mag1c_workspace_doubles(G, S, n), dtype=torch.float64, device=DEV)
    status = torch.full((G,), UNTOUCHED, dtype=torch.int32, device=DEV)
    a = _lib.sc_mag1c_args()
    a.x, a.x_is_f64 = xp.data_ptr(), is64
    a.xoff, a.P, a.Ppad, a.poff = xoff_d.data_ptr(), P_d.data_ptr(), ppad_d.data_ptr(), poff_d.data_ptr()
    a.G, a.S, a.npix = G, S, n
    a.templ = templ.data_ptr()
    a.num_iter, a.alpha, a.cov_update_scaling = int(num_iter), float(alpha), float(k)
    a.albedo_override, a.zero_override, a.sparse_override, a.apply_scaling = (int(f) for f in flags)
    a.work, a.mf_out, a.albedo_out, a.status = work.data_ptr(), mf.data_ptr(), alb.data_ptr(), status.data_ptr()
    _lib.check(lib.sc_mag1c_groups(C.byref(a), st))
    torch.cuda.synchronize()
    mf, alb = mf.cpu().numpy(), alb.cpu().numpy()
    assert np.isnan(mf[n:]).all() and np.isnan(alb[n:]).all(), "written behind the last pixel"
    return mf[:n], alb[:n], status.cpu().numpy()


def nan_in_lds():
    """Leaves NaN all over the LDS of every CU, so that a kernel of the next launch which reads LDS it has not written computes NaN
    (0 * NaN included) where stale finite bits would have gone unnoticed: 512 groups of constant radiance -- zero variance, the first
    pivot is 0 and NaN spreads through the whole 128 x 128 matrix -- through the fp32 resident kernel and through k_mag1c_fast.
    Error-status path only: every group reports status 1."""
    G, P, S = 512, 16, 128
    for dt in ("f32", "f64"):
        status = run_packed(np.full((G * P, S), 3.0, dtype=NP_DT[dt]), (P,) * G, np.full(S, -0.3), alpha=0.0)[2]
        assert (status == 1).all()


@functools.lru_cache(maxsize=None)
def oracle_groups(S, dt, alpha, sizes, singular=-1):
    """radiances of the groups in the element type `dt` and the float64 oracle of every group (None for a skipped one and for the
    group `singular`, whose band 0 is made constant: zero variance, the first pivot of its covariance is exactly 0)"""
    n = sum(sizes)
    x, t = radiances(S, n, 1000 * S + 7 * len(sizes) + n + (dt == "f64"))
    x = x.astype(NP_DT[dt])
    want, o = [], 0
    for gi, p in enumerate(sizes):
        if gi == singular:
            x[o:o + p, 0] = 3.0
        want.append(None if p == 0 or gi == singular else mag1c_ref.acrwl1mf_group(x[o:o + p].astype(np.float64), t, num_iter=30, alpha=alpha))
        o += p
    x.setflags(write=False)
    return x, t, want


def compare_groups(code, dt, sizes, got, want, status, singular=-1):
    mf, alb, _ = got
    o, worst = 0, {}
    for gi, p in enumerate(sizes):
        sl = slice(o, o + p)
        o += p
        if p == 0:
            assert status[gi] == UNTOUCHED, (gi, status)
            continue
        if gi == singular:
            assert status[gi] == 1, (gi, status)
            continue
        assert status[gi] == 0, (gi, status)
        wmf, walb = want[gi]
        assert (wmf > 0).any(), "the case tests nothing: the oracle's result is identically zero"
        assert np.isfinite(mf[sl]).all() and np.isfinite(alb[sl]).all(), (gi, p)
        e, ea = float(rel(mf[sl], wmf).max()), float(rel(alb[sl], walb).max())
        worst[f"{gi}:{p}"] = e
        note(code, e)
        assert e < TOL_MF[dt] and ea < TOL_ALB, (gi, p, e, ea, worst)
    return worst


@pytest.mark.parametrize("case", GROUP_CASES, ids=group_id)
def test_groups_vs_fp64_oracle(hip, case):
    """several groups of ONE launch in mixed order with a skipped group (P = 0) in the middle: every pixel of every group against the
    float64 oracle; the skipped group's status stays untouched, nothing is written behind the last pixel"""
    name, S, dt, alpha, sizes = case
    assert variant(S, dt, alpha) == L[name]
    nan_in_lds()
    x, t, want = oracle_groups(S, dt, alpha, sizes)
    got = run_packed(x, sizes, t, alpha=alpha)
    worst = compare_groups(L[name], dt, sizes, got, want, got[2])
    print(f"{group_id(case)} (code {L[name]}): worst relative error per group {worst}")


# ------------------------------------------------------------------------------------------------ singular groups
# (code, S, element type, pixels per group, index of the group with P <= S); alpha = 0: any shrinkage makes the matrix definite
SINGULAR_CASES = [
    ("TILE4", 24, "f32", (54, 20, 0, 600), 1),
    ("TILE8_PAIR", 80, "f32", (110, 300, 70, 0, 513), 2),          # 70 <= 512 pixels: the resident kernel's flag
    ("F64_FAST", 80, "f64", (110, 70, 0, 1025), 1),
]


@pytest.mark.parametrize("case", SINGULAR_CASES, ids=lambda c: f"{c[0]}-S{c[1]}-{c[2]}")
def test_singular_group_is_flagged_alone(hip, case):
    """one group with P <= S pixels (covariance of rank < S) among well-posed ones.  Rounding can leave a rank-deficient matrix with
    tiny POSITIVE pivots, in the reference as here, so the group also gets a band of constant radiance 3.0: its mean is exact, its
    variance exactly zero and the first pivot is not positive in any arithmetic.  status flags that group and no other, every other
    group matches the oracle, and the Python entry point raises what the reference's torch.linalg.cholesky raises.  (The kernels only
    set a flag on this path: no value of the factorisation reaches an index or a loop bound.)"""
    name, S, dt, sizes, bad = case
    assert variant(S, dt, 0.0) == L[name] and sizes[bad] <= S
    nan_in_lds()
    x, t, want = oracle_groups(S, dt, 0.0, sizes, bad)
    got = run_packed(x, sizes, t, alpha=0.0)
    assert [int(s) for s in got[2]] == [UNTOUCHED if p == 0 else int(gi == bad) for gi, p in enumerate(sizes)]
    compare_groups(L[name], dt, sizes, got, want, got[2], singular=bad)
    o = sum(sizes[:bad])
    with pytest.raises(torch.linalg.LinAlgError):
        hip_mag1c.acrwl1mf(torch.from_numpy(x[None, o:o + sizes[bad]].copy()).to(DEV), t, num_iter=30, alpha=0.0)


# ------------------------------------------------------------------------------------------------ option flags
# (code, element type, S, P, alpha): the resident kernel (300 <= 512 pixels), the streaming kernel of the pair (700), the fp64 kernels
FLAG_CASES = [
    ("TILE8_PAIR", "f32", 80, 300, 0.0), ("TILE8_PAIR_SHRINK", "f32", 80, 300, 1e-4),
    ("TILE8_PAIR", "f32", 80, 700, 0.0), ("TILE8_PAIR_SHRINK", "f32", 80, 700, 1e-4),
    ("F64_FAST", "f64", 80, 700, 0.0), ("F64_1024", "f64", 80, 700, 1e-4),
]
OPTIONS = [
    ("acrwl1mf", dict(albedo_override=True)), ("acrwl1mf", dict(zero_override=True)), ("acrwl1mf", dict(sparse_override=True)),
    ("acrwl1mf", dict(covariance_update_scaling=0.5)), ("rmf", dict(apply_scaling=False)), ("rmf", dict(zero_override=True)),
    ("acrwl1mf", dict(mask=True)),
]


def stat_mask(P, seed):
    """a statistics mask with 16-pixel rows that are fully masked, fully kept and partly masked"""
    m = np.random.default_rng(seed).uniform(size=P) > 0.3
    m[32:64] = False
    m[64:80] = True
    rows = m[:P // 16 * 16].reshape(-1, 16).sum(axis=1)
    assert (rows == 0).sum() >= 2 and (rows == 16).any() and ((rows > 0) & (rows < 16)).sum() >= 4
    return m


@pytest.mark.parametrize("case", FLAG_CASES, ids=lambda c: f"{c[0]}-{c[1]}-S{c[2]}-P{c[3]}")
def test_option_flags_vs_fp64_oracle(hip, case):
    """every option of acrwl1mf / rmf and a statistics mask through the resident kernel, the streaming kernel of the pair and the
    fp64 kernels at 80 bands.  acrwl1mf(zero_override=True) runs with alpha != 0 only: the unclipped rmf result removes the matched
    direction from every pixel exactly, so the first iteration's covariance is singular in exact arithmetic and only the shrinkage
    makes it definite (the oracle raises for alpha = 0); at alpha = 0 the flag is checked through rmf, where it shows as mf < 0"""
    name, dt, S, P, alpha = case
    assert variant(S, dt, alpha) == L[name]
    nan_in_lds()
    B = 2
    x, t = radiances(S, B * P, 77 * S + P + (dt == "f64"))
    x = x.astype(NP_DT[dt]).reshape(B, P, S)
    xd = torch.from_numpy(x).to(DEV)
    mask = stat_mask(P, P)
    worst = {}
    for fn, kw in OPTIONS:
        if fn == "acrwl1mf" and kw.get("zero_override") and alpha == 0.0:
            continue
        kw = dict(kw)
        okw = dict(kw)
        if "mask" in kw:
            kw["mask"], okw["mask"] = torch.from_numpy(mask).to(DEV), mask
        with launches() as rec:
            mf, alb = getattr(hip_mag1c, fn)(xd, t, alpha=alpha, **kw)
        assert rec.codes == [L[name]], (fn, kw, rec.codes)
        wmf, walb = getattr(mag1c_ref, fn)(x.astype(np.float64), t, alpha=alpha, **okw)
        assert (wmf > 0).any() and mf.dtype == xd.dtype
        if kw.get("zero_override") and fn == "rmf":
            assert (wmf < 0).any()
        e, ea = float(rel(mf.cpu().numpy(), wmf).max()), float(rel(alb.cpu().numpy(), walb).max())
        worst[fn + ":" + ",".join(sorted(okw))] = e
        note(L[name], e)
        assert e < TOL_MF[dt] and ea < TOL_ALB, (fn, okw.keys(), e, ea)
    print(f"{name} (code {L[name]}) S={S} P={P} {dt}: worst relative error per option {worst}")


# ------------------------------------------------------------------------------------------------ compute_energy
# (code, element type, S, P, alpha); the fp64 alpha = 0 case is k_mag1c_fast itself: it branches on energy != NULL at run time
ENERGY_CASES = [
    ("TILE4_ENERGY", "f32", 64, 1024, 0.0), ("TILE4_ENERGY", "f32", 17, 1025, 0.0), ("TILE4_ENERGY", "f32", 64, 1025, 0.0),
    ("TILE4_ENERGY_SHRINK", "f32", 64, 1024, 1e-4), ("TILE4_ENERGY_SHRINK", "f32", 17, 1025, 1e-4), ("TILE4_ENERGY_SHRINK", "f32", 64, 1025, 1e-4),
    ("TILE8_ENERGY", "f32", 80, 1024, 0.0), ("TILE8_ENERGY", "f32", 65, 1025, 0.0),
    ("TILE8_ENERGY_SHRINK", "f32", 80, 1024, 1e-4), ("TILE8_ENERGY_SHRINK", "f32", 65, 1025, 1e-4),
    ("F64_512_ENERGY", "f64", 64, 512, 1e-4), ("F64_512_ENERGY", "f64", 17, 1025, 1e-4),
    ("F64_1024_ENERGY", "f64", 80, 512, 1e-4), ("F64_1024_ENERGY", "f64", 65, 1025, 1e-4),
    ("F64_FAST", "f64", 65, 1025, 0.0),
]


@pytest.mark.parametrize("case", ENERGY_CASES, ids=lambda c: f"{c[0]}-{c[1]}-S{c[2]}-P{c[3]}-a{c[4]}")
def test_compute_energy_vs_fp64_oracle(hip, case):
    """compute_energy=True of rmf / acrwl1mf beyond one 512-pixel chunk, with and without a statistics mask, as test_compute_energy
    compares them: the rmf scalar within 2e-6, the per-iteration terms within 2e-5, mf and albedo on every pixel"""
    name, dt, S, P, alpha = case
    assert variant(S, dt, alpha, energy=True) == L[name]
    nan_in_lds()
    B = 2
    x, t = radiances(S, B * P, 31 * S + P + (dt == "f64"))
    x = x.astype(NP_DT[dt]).reshape(B, P, S)
    xd = torch.from_numpy(x).to(DEV)
    mask = stat_mask(P, P + 1)
    for mk in (None, mask):
        kw = {} if mk is None else {"mask": torch.from_numpy(mk).to(DEV)}
        okw = {} if mk is None else {"mask": mk}
        with launches() as rec:
            mf, R, e = hip_mag1c.rmf(xd, t, alpha=alpha, compute_energy=True, **kw)
            mf2, R2, el = hip_mag1c.acrwl1mf(xd, t, num_iter=6, alpha=alpha, compute_energy=True, **kw)
        assert rec.codes == [L[name], L[name]], rec.codes
        wmf, wR, we = mag1c_ref.rmf(x.astype(np.float64), t, alpha=alpha, compute_energy=True, **okw)
        wmf2, wR2, wel = mag1c_ref.acrwl1mf(x.astype(np.float64), t, num_iter=6, alpha=alpha, compute_energy=True, **okw)
        assert (wmf > 0).any() and (wmf2 > 0).any()
        e1, e2 = float(rel(mf.cpu().numpy(), wmf).max()), float(rel(mf2.cpu().numpy(), wmf2).max())
        note(L[name], max(e1, e2))
        got, want = np.array([float(v) for v in el]), np.array(wel)
        ee, eit = abs(float(e) - we) / abs(we), float(np.max(np.abs(got - want) / np.abs(want)))
        print(f"{name} (code {L[name]}) S={S} P={P} {dt} mask={mk is not None}: mf {e1:.2e} / {e2:.2e}, rmf energy {ee:.2e}, iteration terms {eit:.2e}")
        assert e1 < TOL_MF[dt] and e2 < TOL_MF[dt], (e1, e2)
        assert float(rel(R.cpu().numpy(), wR).max()) < TOL_ALB and float(rel(R2.cpu().numpy(), wR2).max()) < TOL_ALB
        assert ee <= 2e-6, (float(e), we)
        assert len(el) == 7 and eit < 2e-5, (got, want)


# ------------------------------------------------------------------------------------------------ DIRECT mode
# (code, S, rows, group id per column, NODATA holes (row0, row1, column, band of the cube), alpha).  The filter's bands are
# [4, 4 + S) of a cube of S + 9 bands.  Plain: column groups of exactly 512 pixels (2 x 256) around a skipped column (6 valid pixels)
DIRECT_CASES = [
    ("TILE8_DIRECT", 128, 256, (1, 1, 2, 3, 3), ((0, 250, 2, 10), (7, 9, 0, 1)), 0.0),
    ("TILE8_DIRECT_SHRINK", 128, 256, (1, 1, 2, 3, 3), ((0, 250, 2, 10), (7, 9, 0, 1)), 1e-4),
    ("TILE8_DIRECT", 65, 250, (1, 2, 2, 3), ((5, 8, 0, 12), (7, 9, 3, 1)), 0.0),
    ("TILE8_DIRECT_SHRINK", 65, 250, (1, 2, 2, 3), ((5, 8, 0, 12), (7, 9, 3, 1)), 1e-4),
]
BAND0 = 4


@functools.lru_cache(maxsize=None)
def direct_scene(S, H, ids, holes):
    W, S_total = len(ids), S + 9
    rng = np.random.default_rng(900 + S + H)
    t = -np.abs(rng.standard_normal(S)) * 0.3
    base = rng.uniform(1, 6, size=S_total)
    cube = base * (1 + 0.05 * rng.standard_normal((H, W, S_total))) + 0.2 * rng.standard_normal((H, W, 1)) * base
    conc = np.zeros(H * W); conc[::7] = 1500.0
    cube[..., BAND0:BAND0 + S] *= 1 + conc.reshape(H, W, 1) * 1e-5 * t
    cube = cube.astype(np.float32)
    for r0, r1, c, b in holes:
        cube[r0:r1, c, b] = hip_mag1c.NODATA
    groups = np.repeat(np.asarray(ids)[None, :], H, 0)
    cube.setflags(write=False)
    return cube, t, groups


def direct_sizes(case):
    """pixels per group as the driver lays them out (a group of <= 10 valid pixels is skipped: 0)"""
    _, S, H, ids, holes, _ = case
    cube, _, groups = direct_scene(S, H, ids, holes)
    valid = np.all(cube[..., BAND0:BAND0 + S] > hip_mag1c.NODATA, axis=-1)
    sizes = [int((valid & (groups == g)).sum()) for g in sorted(set(ids))]
    return tuple(p if p > 10 else 0 for p in sizes)


def by_groups(x, t, groups, alpha, sl, direct_tiles):
    hip_mag1c.DIRECT_TILES = direct_tiles
    try:
        with launches() as rec:
            mf, alb = hip_mag1c.acrwl1mf_by_groups(x, t, groups, alpha=alpha, band_slice=sl)
    finally:
        hip_mag1c.DIRECT_TILES = True
    return mf, alb, rec.codes


@pytest.mark.parametrize("case", DIRECT_CASES, ids=lambda c: f"{c[0]}-S{c[1]}-H{c[2]}")
def test_direct_mode_vs_fp64_oracle(hip, case):
    """DIRECT mode through acrwl1mf_by_groups(band_slice=...): S bands out of a wider cube with band0 > 0; every pixel against the
    float64 oracle, the NODATA pattern exact, and bit-identical with the packed path (DIRECT_TILES = False)"""
    name, S, H, ids, holes, alpha = case
    assert variant(S, "f32", alpha, direct=True) == L[name]
    nan_in_lds()
    cube, t, groups = direct_scene(S, H, ids, holes)
    sl = slice(BAND0, BAND0 + S)
    x = torch.from_numpy(cube.copy()).to(DEV)
    mf, alb, codes = by_groups(x, t, groups, alpha, sl, True)
    assert codes == [L[name]], codes
    pmf, palb, pcodes = by_groups(x, t, groups, alpha, sl, False)
    assert pcodes == [variant(S, "f32", alpha)] and torch.equal(mf, pmf) and torch.equal(alb, palb)
    want, walb = mag1c_ref.func_by_groups(lambda xg: mag1c_ref.acrwl1mf_group(xg, t, num_iter=30, alpha=alpha),
                                          cube[..., sl].astype(np.float64), groups)
    mf, alb = mf.cpu().numpy(), alb.cpu().numpy()
    ok = want != hip_mag1c.NODATA
    assert np.array_equal(mf == hip_mag1c.NODATA, ~ok) and np.array_equal(alb == hip_mag1c.NODATA, ~ok)
    for r0, r1, c, b in holes:                                   # a hole inside the band slice is NODATA, one outside of it is not
        assert bool(ok[r0:r1, c].any()) == (not BAND0 <= b < BAND0 + S)
    worst = {}
    for g in sorted(set(ids)):
        sel = ok & (groups == g)
        if sel.any():
            assert (want[sel] > 0).any()
            worst[g] = float(rel(mf[sel], want[sel]).max())
            note(L[name], worst[g])
            assert worst[g] < TOL_MF["f32"] and rel(alb[sel], walb[sel]).max() < TOL_ALB, (g, worst)
    print(f"{name} (code {L[name]}) S={S} groups of {direct_sizes(case)} pixels: worst relative error per group {worst}")


FALLBACK_SIZES = (300, 513, 200, 95, 5)


def test_direct_mode_falls_back_on_a_513_pixel_group(hip):
    """an arbitrary (non-column) group map whose mean group is small: the direct launch is tried, the 513-pixel group reports
    status 2 and the call is redone by the packed pair -- and still matches the oracle on every pixel, bit-identical with
    DIRECT_TILES = False; the group of 5 pixels stays NODATA"""
    S, alpha, sizes = 65, 0.0, FALLBACK_SIZES
    n = sum(sizes)
    x, t = radiances(S, n, 4242)
    cube = x.astype(np.float32)[None]
    perm = np.random.default_rng(5).permutation(n)
    groups = np.repeat(np.arange(1, len(sizes) + 1), sizes)[perm][None, :]
    xd = torch.from_numpy(cube).to(DEV)
    mf, alb, codes = by_groups(xd, t, groups, alpha, None, True)
    assert codes == [L["TILE8_DIRECT"], L["TILE8_PAIR"]], codes
    pmf, palb, pcodes = by_groups(xd, t, groups, alpha, None, False)
    assert pcodes == [L["TILE8_PAIR"]] and torch.equal(mf, pmf) and torch.equal(alb, palb)
    want, walb = mag1c_ref.func_by_groups(lambda xg: mag1c_ref.acrwl1mf_group(xg, t, num_iter=30, alpha=alpha), cube.astype(np.float64), groups)
    mf, alb = mf.cpu().numpy(), alb.cpu().numpy()
    ok = want != hip_mag1c.NODATA
    assert np.array_equal(mf == hip_mag1c.NODATA, ~ok) and (mf[groups == 5] == hip_mag1c.NODATA).all() and (want[ok] > 0).any()
    e = float(rel(mf[ok], want[ok]).max())
    note(L["TILE8_PAIR"], e)
    assert e < TOL_MF["f32"] and rel(alb[ok], walb[ok]).max() < TOL_ALB


# ------------------------------------------------------------------------------------------------ the tables against the rule
def table_codes():
    """every code a case of this module asserts"""
    return ({L[c[0]] for c in GROUP_CASES} | {L[c[0]] for c in SINGULAR_CASES} | {L[c[0]] for c in FLAG_CASES}
            | {L[c[0]] for c in ENERGY_CASES} | {L[c[0]] for c in DIRECT_CASES} | {L["TILE8_DIRECT"], L["TILE8_PAIR"]})


def swept_codes():
    """every code sc_mag1c_variant returns over the arguments sc_mag1c_groups accepts (and -1 for those it refuses)"""
    lib = _lib.load()
    return {lib.sc_mag1c_variant(S, f64, a0, en, di) for S in range(0, 130) for f64 in (0, 1) for a0 in (0, 1) for en in (0, 1) for di in (0, 1)}


def test_cases_assert_every_code_of_the_rule(hip):
    got = swept_codes()
    assert -1 in got
    assert table_codes() == got - {-1} == set(L.values())


def test_worst_error_per_code(hip):
    """(after the cases above) the worst relative error of mf per variant code"""
    names = {v: k for k, v in L.items()}
    for code in sorted(WORST):
        print(f"code {code} {names[code]}: worst relative error of mf {WORST[code]:.2e}")
