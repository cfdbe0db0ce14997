"""Every token row of the CLIP text tower (mldhip_text_encode) on the MI355X against transformers' CLIPTextModelWithProjection in float64.

The tower is causal and pools at the eos_pos the caller passes, so the P prompts (same id row, eos_pos = 0 .. P - 1) of ONE call return every
row of the tower (tests/clip_tower_ref.py reference_rows / prefix_call).  The rule is clip_tower_ref's, per row: MLDHIP_PREC_F32 within
4 x e32 of fp64, MLDHIP_PREC_F16X3 within 16 x e32, e32 = the float32-CPU error of the same model over the same rows -- or bit equality.
Two layers at the real widths, clip_max_prompts 80.  With MLDHIP_TEXT_TOWER_ROWS_JSON set, the measured values are written there (the
record under profiles/)."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytest.importorskip("transformers")

import clip_tower_ref as R  # noqa: E402
from mld_hip import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

LAYERS, MAXP = 2, 80
ALL = list(range(1, R.CTX + 1))                                  # token rows per prompt: every prefix of the id row
EDGES = [1, 16, 17, 32, 33, 48, 49, 64, 65, 77]                  # key-tile edges, the x3 P V block edges, the fifth tile (wave 0's second), the full context
REGIME_ROWS = [1, 2, 16, 17, 32, 33, 49, 65, 77]
FACTOR = {0: R.F32_FACTOR, 1: R.X3_FACTOR}
MODE = {0: "f32", 1: "f16x3"}


@pytest.fixture(scope="module")
def record():
    rec = {"layers": LAYERS, "f32_factor": R.F32_FACTOR, "x3_factor": R.X3_FACTOR, "probe_tol": _lib.PROBE_TOL}
    yield rec
    dump = os.environ.get("MLDHIP_TEXT_TOWER_ROWS_JSON")
    if dump:
        json.dump(rec, open(dump, "w"), indent=1)


@pytest.fixture(scope="module")
def ids_row():
    return R.make_ids([R.CTX - 1], seed=31)[0]


@pytest.fixture(scope="module")
def reference(ids_row):
    return R.reference_rows(LAYERS, ids_row)


def make_engine(prec, layers=LAYERS, ctx=R.CTX, variant="plain", probe=None):
    eng = _lib.Engine(device=0, precision=prec, **R.engine_kwargs(layers, MAXP, ctx=ctx))
    if probe is not None:
        eng.set_option("range_probe", probe)
    assert R.load_tower(eng, layers, ctx=ctx, variant=variant) == []
    return eng


@pytest.fixture(scope="module")
def engines():
    out = {prec: make_engine(prec) for prec in (0, 1)}
    yield out
    for eng in out.values():
        eng.close()


def encode(eng, ids, eos):
    out = torch.full((len(eos), 1, R.WIDTH), float("nan"), device="cuda:0")
    eng.text_encode(ids, eos, out, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out[:, 0].cpu().numpy()


def rows_of(eng, ids_row, lengths):
    return encode(eng, *R.prefix_call(ids_row, lengths))


def check_rows(out, r64, r32, lengths, prec, what, factor=None):
    """the rule, per row; returns (worst ratio, its n, e32)"""
    err, e32 = R.row_ratios(out, r64, r32, lengths)
    worst = int(np.argmax(err))
    ratio = float(err[worst] / e32) if e32 > 0 else float("inf")
    print(f"{what} [{MODE[prec]}]: e32 {e32:.3e}  worst row n = {lengths[worst]}: {err[worst]:.3e} = {ratio:.2f} x e32")
    factor = FACTOR[prec] if factor is None else factor
    assert e32 > 0 and np.isfinite(out).all(), what
    bad = [(lengths[i], float(err[i] / e32)) for i in range(len(lengths)) if not err[i] <= factor * e32]
    assert not bad, f"{what} [{MODE[prec]}]: rows (n, ratio) above {factor} x e32 = {factor * e32:.3e}: {bad}"
    return ratio, lengths[worst], e32


@pytest.fixture(scope="module")
def all_rows(engines, ids_row):
    """test 1's call: all 77 prefixes at once (3 003 packed rows, 77 unique prompts), per mode"""
    return {prec: rows_of(eng, ids_row, ALL) for prec, eng in engines.items()}


def test_every_row_both_modes(all_rows, reference, engines, record):
    r64, r32 = reference
    for prec in (0, 1):
        ratio, n, e32 = check_rows(all_rows[prec], r64, r32, ALL, prec, "every row, 77 prefixes in one call")
        record.setdefault("every_row", {})[MODE[prec]] = {"e32": e32, "worst_ratio": ratio, "worst_n": n}
        assert engines[prec].numeric_status()["nonfinite_values"] == 0


@pytest.mark.parametrize("prec", [0, 1])
def test_rows_do_not_depend_on_packing(engines, ids_row, all_rows, prec):
    eng, want = engines[prec], all_rows[prec]
    for n in EDGES:                                               # one prompt per call
        assert np.array_equal(rows_of(eng, ids_row, [n])[0], want[n - 1]), n
    perm = [int(n) for n in np.random.default_rng(5).permutation(ALL)]
    for chunk in (perm[:40], perm[40:]):                          # every prompt twice, interleaved A, B, A, C, B, D, C, ...: 40 / 37 unique prompts in 80 / 74
        seq = [chunk[0]]
        for a, b in zip(chunk[:-1], chunk[1:]):
            seq += [b, a]
        seq.append(chunk[-1])
        assert sorted(seq) == sorted(chunk * 2) and len(seq) <= MAXP
        out = rows_of(eng, ids_row, seq)
        for row, n in zip(out, seq):
            assert np.array_equal(row, want[n - 1]), (n, seq)


@pytest.mark.parametrize("prec", [0, 1])
def test_gemm_row_tails(engines, ids_row, all_rows, prec):
    """packed totals on both sides of the 64-row GEMM tile edge (and the one-row call): every row to the bit what the 3 003-row call gave"""
    for total, lengths in {1: [1], 63: [30, 33], 64: [47, 17], 65: [16, 49], 127: [77, 50], 128: [77, 35, 16], 129: [77, 50, 2]}.items():
        assert sum(lengths) == total
        out = rows_of(engines[prec], ids_row, lengths)
        for row, n in zip(out, lengths):
            assert np.array_equal(row, all_rows[prec][n - 1]), (total, n)


def test_context_of_80(record):
    """clip_ctx = 80 (what mldhip_create allows; all five 16-key tiles full): one layer, the last four rows"""
    ctx, lengths = 80, [77, 78, 79, 80]
    row = R.make_ids([ctx - 1], seed=32, ctx=ctx)[0]
    r64, r32 = R.reference_rows(1, row, ctx=ctx)
    for prec in (0, 1):
        eng = make_engine(prec, layers=1, ctx=ctx)
        try:
            ratio, n, e32 = check_rows(rows_of(eng, row, lengths), r64, r32, lengths, prec, "clip_ctx 80")
            record.setdefault("ctx80", {})[MODE[prec]] = {"e32": e32, "worst_ratio": ratio, "worst_n": n}
        finally:
            eng.close()


@pytest.mark.parametrize("variant", ["sharp", "sink", "outlier", "gelu_tails", "gelu_overflow"])
def test_weight_regimes(ids_row, record, variant):
    r64, r32 = R.reference_rows(LAYERS, ids_row, variant=variant)
    # the reference must be informative before the engine is judged by it
    assert np.isfinite(r32).all() and np.isfinite(r64).all()
    peak, key0 = R.attention_shape(LAYERS, ids_row, variant=variant)
    pre, act = R.mlp_peaks(LAYERS, ids_row, variant=variant)
    print(f"{variant}: last-row softmax peak {peak:.3f}, share of rows led by key 0 {key0:.2f}, max|fc1 out| {pre:.1f}")
    if variant in ("sharp", "sink"):
        assert peak > 0.5
    if variant == "sink":
        assert key0 > 0.5
    if variant == "gelu_overflow":
        assert 1.702 * pre > 89.0                                 # expf overflows to inf from 88.73 up
    rec = record.setdefault("regimes", {}).setdefault(variant, {"softmax_peak_last_row": peak, "key0_share": key0, "max_abs_fc1_out": pre})
    for prec in (0, 1):
        eng = make_engine(prec, variant=variant)
        try:
            ns = eng.numeric_status()
            ratio, n, e32 = check_rows(rows_of(eng, ids_row, REGIME_ROWS), r64, r32, REGIME_ROWS, prec, variant)
            rec[MODE[prec]] = {"e32": e32, "worst_ratio": ratio, "worst_n": n}
            if prec == 1:
                print(f"{variant}: probe_err_text {ns['probe_err_text']:.3e}  text_split_ok {ns['text_split_ok']}")
                rec["probe_err_text"], rec["text_split_ok"] = ns["probe_err_text"], ns["text_split_ok"]
                assert ns["probed"] == 1 and ns["text_split_ok"] == (1 if ns["probe_err_text"] <= _lib.PROBE_TOL else 0), ns
            assert eng.numeric_status()["nonfinite_values"] == 0
        finally:
            eng.close()


@pytest.mark.parametrize("variant", ["small_w", "overflow"])
def test_range_contract_fallback(ids_row, record, variant):
    """weights outside the split-f16 format's comfort zone: the probe reads the tower above MLDHIP_PROBE_TOL, the handle says so and returns
    MLDHIP_PREC_F32's numbers"""
    r64, r32 = R.reference_rows(LAYERS, ids_row, variant=variant)
    assert np.isfinite(r32).all()
    if variant == "overflow":
        assert R.mlp_peaks(LAYERS, ids_row, variant=variant)[1] > 65504.0
    exact, split = make_engine(0, variant=variant), make_engine(1, variant=variant)
    try:
        ns = split.numeric_status()
        print(f"{variant}: probe_err_text {ns['probe_err_text']:.3e}  text_split_ok {ns['text_split_ok']}")
        record.setdefault("range_contract", {})[variant] = {"probe_err_text": ns["probe_err_text"] if np.isfinite(ns["probe_err_text"]) else "inf",
                                                            "text_split_ok": ns["text_split_ok"]}
        assert ns["probed"] == 1 and ns["text_split_ok"] == 0 and not ns["probe_err_text"] <= _lib.PROBE_TOL, ns
        want, got = rows_of(exact, ids_row, REGIME_ROWS), rows_of(split, ids_row, REGIME_ROWS)
        assert np.array_equal(got, want)
        ratio, n, e32 = check_rows(got, r64, r32, REGIME_ROWS, 1, variant + " (fell back)", factor=R.F32_FACTOR)
        record["range_contract"][variant].update(e32=e32, worst_ratio=ratio, worst_n=n)
        assert split.numeric_status()["nonfinite_values"] == 0
    finally:
        exact.close()
        split.close()


def test_range_contract_counter_without_the_probe(ids_row, record):
    """contract part 3: with "range_probe" 0 nothing falls back, and a hidden activation beyond the half range must show -- non-finite
    output rows, counted by mldhip_numeric_status (NaN values, not a GPU fault)"""
    assert R.mlp_peaks(LAYERS, ids_row, variant="overflow")[1] > 65504.0
    eng = make_engine(1, variant="overflow", probe=0)
    try:
        ns = eng.numeric_status()
        assert ns["probed"] == 0 and ns["text_split_ok"] == 1 and ns["probe_err_text"] == -1.0, ns
        out = rows_of(eng, ids_row, REGIME_ROWS)
        n = eng.numeric_status()["nonfinite_values"]
        print(f"overflow, range_probe 0: {int((~np.isfinite(out)).sum())} non-finite output values, counter {n}")
        record["overflow_unguarded_nonfinite_values"] = int(n)
        assert not np.isfinite(out).all() and n > 0
        assert n == int((~np.isfinite(out)).sum())
    finally:
        eng.close()


def test_plain_weights_stay_split(engines, record):
    ns = engines[1].numeric_status()
    print(f"plain: probe_err_text {ns['probe_err_text']:.3e}  text_split_ok {ns['text_split_ok']}")
    record.setdefault("range_contract", {})["plain"] = {"probe_err_text": ns["probe_err_text"], "text_split_ok": ns["text_split_ok"]}
    assert ns["probed"] == 1 and ns["text_split_ok"] == 1 and 0 <= ns["probe_err_text"] <= _lib.PROBE_TOL, ns
    n0 = engines[0].numeric_status()
    assert n0["text_split_ok"] == 0 and n0["probe_err_text"] == -1.0, n0      # the F32 handle: nothing to probe
