"""The text-to-motion metric kernels of the engine (mldhip_t2m_match / mldhip_act_stats / mldhip_pair_dist) on the MI355X against the project's float64
restatement (tests/t2m_metrics_ref.py: the inputs, the restatement and the value, rank and FID rules).  The simulator's cases plus the shapes only hardware
reaches: match at the protocol's 2 048 x 512 in groups of 32, 257 groups (more than CUs) and D = 1024; statistics at (301, 30), (700, 256), the protocol's
(4 640, 512), D = 31 / 32 / 33, the offset case x + 100 at (700, 64) that a one-pass E[xx] - E[x]E[x] kernel fails, and the FID rule at (700, 512) over 8
draws; pair distances at P = 300 and 8 192, D = 512 and 1024; F32 and F16X3 handles bit-equal; and MLD.t2m_eval's embeddings through HipTM2TMetrics on
the model's own handle.  The measured ratios go to the file MLDHIP_T2M_METRICS_JSON names (profiles/t2m_metrics.json is written from such a run)."""
import faulthandler
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import simlib  # noqa: E402
import t2m_metrics_ref as R  # noqa: E402
from mld_hip import _lib  # noqa: E402
from mld_hip import synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu

TIME_LIMIT_S = 120
DEV = "cuda:0"
_record = {}

MATCH = {"N 2048, D 512, R 32": (2048, 512, 32), "N 1028, D 8, R 4 (257 groups)": (1028, 8, 4), "N 64, D 1024, R 32": (64, 1024, 32),
         "N 32, D 512, R 32": (32, 512, 32), "N 23, D 6, R 5": (23, 6, 5), "N 62, D 30, R 31": (62, 30, 31)}
STATS = {"N 301, D 30": (301, 30, 0.0), "N 700, D 256": (700, 256, 0.0), "N 4640, D 512": (4640, 512, 0.0), "N 257, D 31": (257, 31, 0.0),
         "N 256, D 32": (256, 32, 0.0), "N 255, D 33": (255, 33, 0.0), "N 3, D 5": (3, 5, 0.0), "N 2, D 1": (2, 1, 0.0), "N 700, D 64, x + 100": (700, 64, 100.0)}
PAIRS = {f"P {P}, D {D}": (P, D) for P in (300, 8192) for D in (512, 1024)}
PAIRS.update({f"P {P}, D {D}": (P, D) for P in (1, 40) for D in (1, 3)})


@pytest.fixture(autouse=True)
def time_limit():
    """every test of this file ends after TIME_LIMIT_S at the latest, also when it is blocked inside a device synchronisation"""
    faulthandler.dump_traceback_later(TIME_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def engines():
    out = {prec: _lib.Engine(device=0, precision=prec, **R.engine_kwargs()) for prec in (0, 1)}
    yield out
    for eng in out.values():
        eng.close()
    dump = os.environ.get("MLDHIP_T2M_METRICS_JSON")
    if dump:
        json.dump({"rule": "value: err = max|engine - fp64 restatement| <= 4 x e32 = max|torch fp32 CPU restatement - fp64 restatement|; rank: exact on every row "
                           "whose fp64 diagonal is >= 1e-4 from the rest of its row; FID: max over 8 draws of |FID(engine) - FID(fp64)| <= 4 x max |FID(fp32) - FID(fp64)|",
                   "cases": _record}, open(dump, "w"), indent=1)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(*ts):
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


def match(eng, t, m, Rr, **kw):
    return host(*R.run_match(eng, dev(t), dev(m), Rr, stream=torch.cuda.current_stream().cuda_stream, **kw))


def stats(eng, x):
    return host(*R.run_stats(eng, dev(x), stream=torch.cuda.current_stream().cuda_stream))


def pairs(eng, x, a, b):
    return host(R.run_pairs(eng, dev(x), a, b, stream=torch.cuda.current_stream().cuda_stream))[0]


@pytest.fixture(scope="module")
def match_refs():
    """inputs and the float64 restatement of every match case, computed once, shared, left unchanged"""
    out = {}
    for name, (N, D, Rr) in MATCH.items():
        t, m = R.match_inputs(N, D)
        out[name] = (t, m, R.match_reference(t, m, Rr))
    return out


@pytest.mark.parametrize("name", list(MATCH))
def test_match_against_fp64(engines, match_refs, name):
    N, D, Rr = MATCH[name]
    t, m, ref = match_refs[name]
    n = N // Rr * Rr
    top1 = float((ref["rank64"] == 0).mean())
    assert 0.05 < top1 < 0.95
    rank, diag = match(engines[0], t, m, Rr)
    assert (rank[n:] == -7).all() and np.isnan(diag[n:]).all()                 # tail rows: untouched
    R.check_value(diag[:n], (ref["diag64"], ref["e32_diag"]), f"diag, {name}", _record)
    R.check_ranks(rank[:n], ref, name)
    _record[f"rank, {name}"] = dict(rows=n, left_out=int((~ref["counts"]).sum()), top1_fp64=top1, top1_engine=float((rank[:n] == 0).mean()))
    rank1, diag1 = match(engines[1], t, m, Rr)                                  # the F16X3 handle: the same bits
    assert np.array_equal(rank, rank1) and np.array_equal(diag, diag1, equal_nan=True)
    r_only, _ = match(engines[0], t, m, Rr, diag=False)                         # either output may be NULL
    _, d_only = match(engines[0], t, m, Rr, rank=False)
    assert np.array_equal(r_only, rank) and np.array_equal(d_only, diag, equal_nan=True)


def test_match_ties_and_nan(engines, match_refs):
    t, m, _ = match_refs["N 62, D 30, R 31"]
    rank, diag = match(engines[0], *R.tie_case(t, m), 31)
    R.check_ties(rank)
    rank, diag = match(engines[0], *R.nan_case(t, m), 31)
    R.check_nan_row(rank, diag)


@pytest.fixture(scope="module")
def stats_outs(engines):
    out = {}
    for name, (N, D, off) in STATS.items():
        x = R.stats_inputs(N, D, offset=off)
        out[name] = (x, R.stats_reference(x), stats(engines[0], x))
    return out


@pytest.mark.parametrize("name", list(STATS))
def test_stats_against_fp64(engines, stats_outs, name):
    x, (rm, rc), (mean, cov) = stats_outs[name]
    R.check_value(mean, rm, f"mean, {name}", _record)
    R.check_value(cov, rc, f"cov, {name}", _record)
    assert np.array_equal(cov, cov.T)                                          # exactly symmetric
    mean1, cov1 = stats(engines[1], x)                                         # the F16X3 handle, and a second call: the same bits
    assert np.array_equal(mean, mean1) and np.array_equal(cov, cov1)


def test_fid_rule(engines):
    R.check_fid(700, 512, lambda x: stats(engines[0], x), "FID, N 700, D 512, 8 draws", _record)


@pytest.mark.parametrize("name", list(PAIRS))
def test_pairs_against_fp64(engines, name):
    P, D = PAIRS[name]
    x, a, b = R.pair_inputs(max(50, P // 2), D, P)
    out = pairs(engines[0], x, a, b)
    R.check_value(out, R.pair_reference(x, a, b), f"dist, {name}", _record)
    if P > 1:
        assert out[0] == 0.0 and a[0] == b[0]                                   # a == b: exactly 0
    assert np.array_equal(out, pairs(engines[1], x, a, b))


def test_capacity_and_guards(engines):
    eng = engines[0]
    x = R.stats_inputs(8193, 4)
    for call in (lambda: stats(eng, x), lambda: match(eng, x, x, 4), lambda: pairs(eng, x, [0], [1])):
        with pytest.raises(_lib.MldHipError) as ei:
            call()
        assert ei.value.code == -1
    with pytest.raises(_lib.MldHipError) as ei:
        pairs(eng, x[:10], [0, 10], [1, 2])                                     # an index behind N, refused on the host
    assert ei.value.code == -1
    plain = _lib.Engine(device=0, num_layers=3, max_batch=1, max_frames=16)
    with pytest.raises(_lib.MldHipError) as ei:
        stats(plain, x[:10])
    assert ei.value.code == -3
    plain.close()


def test_t2m_eval_through_the_metrics():
    """MLD.t2m_eval (synthetic weights, two DDIM steps) -> HipTM2TMetrics / HipMMMetrics on the model's own handle (cfg.model.metric_ops): finite metrics, and
    the match / statistics of the metric's gathered sets within the rules of the float64 restatement."""
    import t2m_ref as T
    from mld_hip import config as C
    from mld_hip import engine as E
    from mld_hip.datamodule import HipDataModule
    from mld_hip.evaluators import HipMetricOps
    from mld_hip.metrics import HipMMMetrics, HipTM2TMetrics
    from mld_hip.mld import MLD
    from mld_hip.text_encoder import SyntheticTextEncoder

    d = torch.device(DEV)
    E.drop_engines()
    E.configure(max_batch=4, max_frames=64)
    over = {"model.denoiser.params.num_layers": simlib.SIM_LAYERS, "model.motion_vae.params.num_layers": simlib.SIM_LAYERS,
            "model.scheduler.num_inference_timesteps": 2, "model.t2m_evaluator.target": "mld_hip.evaluators.HipT2MEvaluator",
            "model.metric_ops.target": "mld_hip.evaluators.HipMetricOps"}
    cfg = C.load_config(overrides=over)
    model = MLD(cfg, HipDataModule(cfg), text_encoder=SyntheticTextEncoder()).to(d).eval()
    assert isinstance(model.metric_ops, HipMetricOps)
    metric = HipTM2TMetrics(top_k=3, R_size=4, diversity_times=5, ops=model.metric_ops)
    mm = HipMMMetrics(mm_num_times=2, ops=model.metric_ops)
    lengths, text_lens, L = [24, 40, 9, 40], [3, 5, 1, 2], 5
    for k in range(3):
        motion = torch.from_numpy(T.make_motions(lengths, 40, seed=31 + k)).to(d)
        w, p = T.make_captions(text_lens, L, seed=40 + k)
        batch = {"text": ["a person walks.", "someone jumps twice.", "a man waves.", "a person sits down."], "motion": motion, "length": lengths,
                 "word_embs": torch.from_numpy(w).to(d), "pos_ohot": torch.from_numpy(p).to(d), "text_len": torch.tensor(text_lens)}
        lat0 = torch.from_numpy(syn.make_batch(4, lengths, seed=50 + k).init_latents).to(d)
        rs = model.t2m_eval(batch, init_latents=lat0)
        metric.update(rs["lat_t"], rs["lat_rm"], rs["lat_m"], lengths)
        mm.update(rs["lat_rm"].unsqueeze(0), lengths[:1])
    assert metric.ops.engine_of(rs["lat_t"]) is model._engine()                 # the model's handle, no second one
    torch.manual_seed(3)
    np.random.seed(3)
    out = metric.compute(sanity_flag=False)
    assert set(out) == set(metric.metrics) and len(out) == 11
    vals = {k: float(v) for k, v in out.items()}
    print("HipTM2TMetrics on MLD.t2m_eval:", vals)
    assert all(np.isfinite(v) for v in vals.values())
    assert 0.0 <= vals["R_precision_top_1"] <= vals["R_precision_top_2"] <= vals["R_precision_top_3"] <= 1.0
    mmv = float(mm.compute(sanity_flag=False)["MultiModality"])
    assert np.isfinite(mmv) and mmv > 0
    _record["MLD.t2m_eval -> HipTM2TMetrics"] = {**vals, "MultiModality": mmv}
    E.drop_engines()
