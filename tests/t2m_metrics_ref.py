"""Shared pieces of the text-to-motion metric tests (tests/test_t2m_metrics_sim.py, tests/test_t2m_metrics_golden.py, tests/test_t2m_metrics.py on the CPU,
tests/test_gpu_t2m_metrics.py on the MI355X; tools/ab_t2m_metrics.py times the host side): the seeded inputs, the project's own restatement of the three
calls mldhip_t2m_match / mldhip_act_stats / mldhip_pair_dist (the math written out in include/mldhip.h) in float64 or float32, and the rules.

The restatement is pinned to the reference's own utils.py by tests/golden/t2m_metrics.npz (tools/make_golden_t2m_metrics.py).

Value rule (the project's F32_FACTOR = 4, as in tests/a2m_rec_ref.py): err = max|engine - float64 restatement|; e32 = max|the same formula in torch float32
on the CPU - float64|; e32 > 0 and err <= 4 e32.  Applied to diag, mean, cov and dist.

Rank rule: a row COUNTS when, in float64, its diagonal is at least GAP = 1e-4 away from every other entry of the row; every counting row carries float64's
rank exactly.  Why 1e-4: the float32-CPU distance error measured on these inputs is at most 1.04e-5, so under the value rule two entries can swap only
inside 2 x 4 x 1.04e-5 = 8.4e-5.  At most 1 % of a case's rows may be left out (at most one row in cases under 100 rows); ``match_reference`` asserts
that cap on the float64 restatement alone, and the seeds below are chosen so that it holds.

FID rule: a scalar's float32 error varies 50-fold from draw to draw, so a per-case ratio is meaningless.  Over FID_DRAWS = 8 seeded draws of one shape:
|FID(engine statistics) - FID(np.cov float64 statistics)| <= 4 x max over the draws of |FID(float32-CPU statistics) - FID(float64 statistics)|."""
import numpy as np
import torch

from mld_hip.metrics import calculate_frechet_distance

F32_FACTOR = 4.0
GAP = 1e-4
CHUNK = 256          # MLDHIP_ACT_STATS_CHUNK (include/mldhip.h)
FID_DRAWS = 8

# alpha per D so that top-1 lands strictly between 5 % and 95 % at R = 32 (D 512: 0.44, D 30: 0.57, D 6: 0.15)
ALPHA = {512: 0.1, 1024: 0.07, 30: 0.5, 8: 0.5, 6: 0.5}


def header_chunk():
    """MLDHIP_ACT_STATS_CHUNK as include/mldhip.h names it"""
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mldhip.h")).read()
    return int(re.search(r"#define MLDHIP_ACT_STATS_CHUNK (\d+)", text).group(1))


def match_inputs(N, D, seed=None, alpha=None):
    """text ~ N(0, 1), motion = alpha text + N(0, 1), float32 [N, D]"""
    g = torch.Generator().manual_seed(1000 * D + N if seed is None else seed)
    text = torch.randn(N, D, generator=g)
    motion = (ALPHA[D] if alpha is None else alpha) * text + torch.randn(N, D, generator=g)
    return text.numpy(), motion.numpy()


def stats_inputs(N, D, seed=None, offset=0.0):
    """correlated Gaussians N(0, 1) @ A + offset with A = N(0, 1) / sqrt(D), float32 [N, D]"""
    g = torch.Generator().manual_seed(1000 * D + N if seed is None else seed)
    A = torch.randn(D, D, generator=g) / D ** 0.5
    return (torch.randn(N, D, generator=g) @ A + offset).float().numpy()


# (under the default seed the one pair of (P 1, D 1) subtracts exactly in float32: e32 = 0 and the value rule has nothing to measure)
PAIR_SEEDS = {(1, 1): 1}


def pair_inputs(N, D, P, seed=None):
    """x float32 [N, D] and index lists a, b [P]; with P > 1, pair 0 has a == b"""
    g = torch.Generator().manual_seed(PAIR_SEEDS.get((P, D), 1000 * D + P + 1) if seed is None else seed)
    x = torch.randn(N, D, generator=g)
    a = torch.randint(0, N, (P,), generator=g).numpy().astype(np.int32)
    b = torch.randint(0, N, (P,), generator=g).numpy().astype(np.int32)
    if P > 1:
        b[0] = a[0]
    return x.numpy(), a, b


# ---------------------------------------------------------------- the restatement (torch, any float dtype)
def dist_matrices(text, motion, R, dtype=torch.float64):
    """[G, R, R]: sqrt(-2 t.m + |t|^2 + |m|^2) of every group, nan_to_num'd (NaN -> 0, +inf -> the dtype's largest value as float32 has it)"""
    t, m = torch.as_tensor(text).to(dtype), torch.as_tensor(motion).to(dtype)
    G = t.shape[0] // R
    t, m = t[:G * R].reshape(G, R, -1), m[:G * R].reshape(G, R, -1)
    d1 = -2 * torch.bmm(t, m.transpose(1, 2))
    d2 = torch.sum(torch.square(t), dim=2, keepdim=True)
    d3 = torch.sum(torch.square(m), dim=2).unsqueeze(1)
    return torch.sqrt(d1 + d2 + d3).nan_to_num(posinf=float(np.finfo(np.float32).max))


def ranks_of(d):
    """rank [G, R] of each row's diagonal entry: #{j: d_ij < d_ii} + #{j < i: d_ij == d_ii}, the position a stable ascending sort gives column i"""
    G, R, _ = d.shape
    dii = torch.diagonal(d, dim1=1, dim2=2).unsqueeze(2)
    before = torch.tril(torch.ones(R, R, dtype=torch.bool), -1).unsqueeze(0)
    return ((d < dii) | ((d == dii) & before)).sum(2)


def match_reference(text, motion, R):
    """dict: d64 [G, R, R], diag64 / e32_diag, rank64 [G R], counts [G R] (the rows of the rank rule); asserts the cap of the rank rule on float64 alone"""
    d64 = dist_matrices(text, motion, R, torch.float64)
    d32 = dist_matrices(text, motion, R, torch.float32)
    G = d64.shape[0]
    diag64 = torch.diagonal(d64, dim1=1, dim2=2)
    off = (d64 - diag64.unsqueeze(2)).abs() + torch.eye(R, dtype=torch.float64).unsqueeze(0) * 1e30
    counts = (off.min(2).values >= GAP).reshape(-1).numpy()
    left = int((~counts).sum())
    assert left <= (0.01 * G * R if G * R >= 100 else 1), (left, G * R)
    # (the float32 CPU agrees with float64 on every counting row: the rule asks nothing a float32 evaluation does not deliver)
    assert np.array_equal(ranks_of(d32).reshape(-1).numpy()[counts], ranks_of(d64).reshape(-1).numpy()[counts])
    return dict(d64=d64.numpy(), diag64=diag64.reshape(-1).numpy(), rank64=ranks_of(d64).reshape(-1).numpy(), counts=counts,
                e32_diag=float((torch.diagonal(d32, dim1=1, dim2=2).double() - diag64).abs().max()))


def stats(x, dtype=torch.float64):
    """(mean [D], cov [D, D]) = column mean and (X - mean)^T (X - mean) / (N - 1), rows centred before they are multiplied"""
    x = torch.as_tensor(x).to(dtype)
    mu = x.mean(0)
    xc = x - mu
    return mu, xc.T @ xc / (x.shape[0] - 1)


def stats_reference(x):
    """((mean64, e32_mean), (cov64, e32_cov))"""
    (m64, c64), (m32, c32) = stats(x, torch.float64), stats(x, torch.float32)
    return (m64.numpy(), float((m32.double() - m64).abs().max())), (c64.numpy(), float((c32.double() - c64).abs().max()))


def pair_dist(x, a, b, dtype=torch.float64):
    x = torch.as_tensor(x).to(dtype)
    a, b = torch.as_tensor(np.asarray(a)).long(), torch.as_tensor(np.asarray(b)).long()
    return torch.sqrt(torch.square(x[a] - x[b]).sum(1))


def pair_reference(x, a, b):
    d64, d32 = pair_dist(x, a, b, torch.float64), pair_dist(x, a, b, torch.float32)
    return d64.numpy(), float((d32.double() - d64).abs().max())


# ---------------------------------------------------------------- the rules
def check_value(out, ref, what, record=None):
    """the value rule; returns err / e32 (and notes it in ``record``)"""
    r64, e32 = ref
    out = np.asarray(out)
    err = float(np.abs(out.astype(np.float64) - r64).max())
    print(f"{what}: err {err:.3e}  e32 {e32:.3e}  ratio {err / e32 if e32 > 0 else float('inf'):.2f}")
    if record is not None:
        record[what] = dict(err=err, e32=e32, ratio=err / e32 if e32 > 0 else None)
    assert np.isfinite(out).all(), what
    assert e32 > 0, what
    assert err <= F32_FACTOR * e32, (what, err, e32)
    return err / e32


def check_ranks(rank, ref, what=""):
    """the rank rule: every counting row carries float64's rank"""
    rank = np.asarray(rank).reshape(-1)
    ok = ref["counts"]
    assert np.array_equal(rank[ok], ref["rank64"][ok]), what


# the tie and NaN cases of the match tests, on the inputs of (N 62, D 30, R 31)
def tie_case(text, motion):
    """motions 5 and 22 of group 0 become copies of motion 12: rows 5, 12 and 22 each see their own distance three times (indices at which every other
    entry of those rows stays GAP away from the diagonal: ``check_ties`` asserts it)"""
    m = motion.copy()
    m[5], m[22] = m[12], m[12]
    return text, m


def check_ties(rank, R=31):
    """a tie LEFT of the diagonal counts, one right of it does not: against the float64 count of strictly smaller entries among the other columns"""
    text, m = tie_case(*match_inputs(62, 30))
    d = dist_matrices(text, m, R)[0].numpy()
    others = np.setdiff1d(np.arange(R), [5, 12, 22])
    for i, ties_left in ((5, 0), (12, 1), (22, 2)):
        smaller = d[i, others] < d[i, i]
        assert np.abs(d[i, others] - d[i, i]).min() >= GAP
        assert rank[i] == int(smaller.sum()) + ties_left, (i, rank[i])


def nan_case(text, motion):
    """one NaN element in text row 40 (group 1, row 9)"""
    t = text.copy()
    t[40, 7] = np.nan
    return t, motion


def check_nan_row(rank, diag):
    """the row's distances are all 0 (nan_to_num), so its rank is its index in the group; every other row stays finite"""
    assert rank[40] == 9 and diag[40] == 0.0
    assert np.isfinite(np.delete(diag, 40)).all()


def fid(mu_a, cov_a, mu_b, cov_b):
    """FID = calculate_frechet_distance(gt_mu, gt_cov, mu, cov) on float64 casts: ``a`` is the ground truth"""
    f = lambda v: np.asarray(v, np.float64)
    return float(calculate_frechet_distance(f(mu_a), f(cov_a), f(mu_b), f(cov_b)))


def fid_draw(N, D, k):
    """draw k of the FID rule: (generated, ground truth) float32 [N, D], two correlated Gaussians a small shift apart"""
    return stats_inputs(N, D, seed=7000 + 2 * k, offset=0.05), stats_inputs(N, D, seed=7001 + 2 * k)


def fid_sides(N, D, stats_fn, draws=FID_DRAWS):
    """(max over the draws of |FID(stats_fn) - FID(np.cov float64)|, max over the draws of |FID(float32-CPU stats) - FID(float64 stats)|); the FID rule is
    left <= 4 right.  ``stats_fn(x)`` -> (mean, cov) of the code under test."""
    left = right = 0.0
    for k in range(draws):
        gen, gt = fid_draw(N, D, k)
        g64, t64 = gen.astype(np.float64), gt.astype(np.float64)
        f64 = fid(t64.mean(0), np.cov(t64, rowvar=False), g64.mean(0), np.cov(g64, rowvar=False))
        (mg, cg), (mt, ct) = stats(gen, torch.float32), stats(gt, torch.float32)
        f32 = fid(mt.numpy(), ct.numpy(), mg.numpy(), cg.numpy())
        (emg, ecg), (emt, ect) = stats_fn(gen), stats_fn(gt)
        fe = fid(emt, ect, emg, ecg)
        left, right = max(left, abs(fe - f64)), max(right, abs(f32 - f64))
    return left, right


def check_fid(N, D, stats_fn, what, record=None, draws=FID_DRAWS):
    left, right = fid_sides(N, D, stats_fn, draws)
    print(f"{what}: |FID(engine) - FID(fp64)| {left:.3e}  max |FID(fp32) - FID(fp64)| {right:.3e}")
    if record is not None:
        record[what] = dict(engine=left, float32=right)
    assert right > 0 and left <= F32_FACTOR * right, (what, left, right)


def engine_kwargs(metrics_max_rows=0, **extra):
    """mldhip_config fields of a small engine that carries the metric kernels (the diffusion model is the 3-layer text stack, never loaded)"""
    return dict(num_layers=3, max_batch=1, max_frames=16, t2m_metrics=1, metrics_max_rows=metrics_max_rows, **extra)


# ---------------------------------------------------------------- thin callers (numpy on the simulator, tensors on the device)
def run_match(eng, text, motion, R, rank=True, diag=True, N=None, stream=0):
    """-> (rank [N] int32 prefilled with -7, diag [N] float32 prefilled with NaN): tail rows must come back untouched"""
    xp_is_np = isinstance(text, np.ndarray)
    N = text.shape[0] if N is None else N
    if xp_is_np:
        ro = np.full(N, -7, np.int32) if rank else None
        do = np.full(N, np.nan, np.float32) if diag else None
    else:
        ro = torch.full((N,), -7, dtype=torch.int32, device=text.device) if rank else None
        do = torch.full((N,), float("nan"), dtype=torch.float32, device=text.device) if diag else None
    eng.t2m_match(text, motion, N, text.shape[1], R, ro, do, stream)
    return ro, do


def run_stats(eng, x, stream=0):
    N, D = x.shape
    if isinstance(x, np.ndarray):
        mean, cov = np.full(D, np.nan, np.float32), np.full((D, D), np.nan, np.float32)
    else:
        mean = torch.full((D,), float("nan"), dtype=torch.float32, device=x.device)
        cov = torch.full((D, D), float("nan"), dtype=torch.float32, device=x.device)
    eng.act_stats(x, N, D, mean, cov, stream)
    return mean, cov


def run_pairs(eng, x, a, b, stream=0):
    if isinstance(x, np.ndarray):
        out = np.full(len(a), np.nan, np.float32)
    else:
        out = torch.full((len(a),), float("nan"), dtype=torch.float32, device=x.device)
    eng.pair_dist(x, x.shape[0], x.shape[1], a, b, out, stream)
    return out


# ---------------------------------------------------------------- the recorded run of tests/golden/t2m_metrics.npz (tools/make_golden_t2m_metrics.py)
GOLD = dict(updates=3, rows=40, D=512, R=32, top_k=3, diversity_times=30, compute_seed=41, mm_texts=6, mm_reps=12, mm_times=5, mm_seed=45)
GOLD_COV_STEP = 8      # the file holds every 8th row and column of the two covariances (and their traces): a 512 x 512 float64 pair would not fit a small fixture


def golden_updates(draw=0):
    """the seeded embeddings of the recorded run (``draw`` 0), not stored in the file: [(text, generated [rows, 1, D], ground truth), ...] float32;
    draws 1 .. 8 are further sets of the same shape and distribution, for the right-hand side of the FID rule at this shape"""
    g = torch.Generator().manual_seed(4100 + draw)
    out = []
    for _ in range(GOLD["updates"]):
        t = torch.randn(GOLD["rows"], GOLD["D"], generator=g)
        gen = 0.1 * t + torch.randn(GOLD["rows"], GOLD["D"], generator=g)
        gt = 0.15 * t + torch.randn(GOLD["rows"], GOLD["D"], generator=g) @ (torch.eye(GOLD["D"]) + 0.02 * torch.randn(GOLD["D"], GOLD["D"], generator=g))
        out.append((t, gen.unsqueeze(1), gt))
    return out


def golden_mm():
    """the multimodality embeddings of the recorded run: mm_texts tensors [1, mm_reps, D]"""
    g = torch.Generator().manual_seed(4200)
    return [torch.randn(1, GOLD["mm_reps"], GOLD["D"], generator=g) for _ in range(GOLD["mm_texts"])]
