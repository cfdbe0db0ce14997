#!/usr/bin/env python
"""motions/sec of the MLD sampling hot path on MI355X (BASELINE.json metric).

  python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]
      N > 1 without torchrun: bench.py re-launches itself as N ranks (python -m torch.distributed.run, 127.0.0.1);
      under torchrun (RANK / WORLD_SIZE set) it is one of the N ranks.

A plain run measures the headline only: set-up, W warm-up steps, ONE timed region of exactly K steps, the result line.  --full adds
every other measurement below (single-batch and pipelined figures, rocprofv3 rooflines, requests-per-call sweep, CPU baseline, parity,
other arithmetic modes, length mix, configs 4 / 5, CLIP tower) and repeats the timed region --repeats times (default 5, median reported).
--dump-outputs DIR writes what the last timed step returned to its caller (latents and joints of that bs-64 request) as float32 .npy files;
the inputs are seeded, so two builds can be compared output for output.

One "step" = one pass of the hot path over one batch: 50-step DDIM latent sampling with classifier-free guidance ->
motion-VAE decode -> (T,22,3) joints for B=64 synthetic HumanML3D-shaped prompts (config_mld_humanml3d.yaml, T=196),
inputs resident in HBM, text embeddings precomputed (the frozen CLIP encoder is outside this path).  The K steps are K
independent bs-64 requests that are all available at t = 0; the serving entry (mldhip_sample_many) takes up to --coalesce of
them (default 32 = 2 048 motions) per call: ONE persistent launch runs the whole reverse loop of the call (a workgroup per 8
motions, kernels/loop_fused.hpp), then one decode.  Calls are issued one after another on ONE stream: no calls in flight, no
stream / hardware-queue placement to get right (round 2's headline needed both).  The timed region (exactly K steps between
barrier + synchronize pairs) is repeated --repeats times; `value` is the median repetition, min / max are carried.  A warm-up
step is one untimed bs-64 request in the timed region's call shapes; every call shape is warmed (its graph captured) at least once.
`single_batch` / `value_single_batch` is the same K steps issued strictly one bs-64 batch after another (the configuration
BASELINE.json's metric names literally; since round 5 the reverse loop of such a call is ONE launch of workgroup clusters,
kernels/loop_cluster.hpp), with its own roofline from a second rocprofv3 child.  Ranks are pure data parallel: weights are broadcast once
from rank 0 (one RCCL broadcast of the packed blob), every rank samples its own prompts, no data-path collective.  Rank 0
prints ONE JSON line.

Arithmetic: the headline runs `--precision f16x3` (split-f16: every GEMM operand x = hi + lo in IEEE half, three
v_mfma_f32_16x16x32_f16 per product with fp32 accumulation, 22 mantissa bits; attention scores / softmax / LayerNorm /
residuals / scheduler in fp32) -- it meets the <= 1e-3 joint tolerance with a 5x margin (tests/test_gpu_parity.py asserts
every motion of this call shape; the measured error is in `parity`).  Exact-fp32 MFMA and plain bf16 are reported as
`alt_modes`, each with its measured error.

roofline: the dominant kernel of the headline call by rocprofv3 time -- `achieved` / `frac` = algorithmic FLOPs per launch / its
average dispatch duration from a rocprofv3 --kernel-trace --stats child run of the same call shape (the summary committed under
profiles/); the live figure (HIP events around loop-only calls on the launch stream) is carried beside it as `frac_hip_events`.  The peak is the one that binds the kernel's arithmetic: split-f16 kernels issue
three f16 MFMAs per algorithmic product, so their roof is the dense f16 MFMA peak / 3; exact-fp32 kernels: the fp32 MFMA peak.
"""
import argparse
import csv
import ctypes as C
import glob
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

# Only the secondary legs (round-2 serving shape, config 4 / 5) put calls in flight on several HIP streams; ROCm multiplexes
# streams onto GPU_MAX_HW_QUEUES (default 4) hardware queues, eight give each of those streams its own (DESIGN.md §3 point 15).
# The headline runs on ONE stream and does not depend on this.  Must be set before the HIP runtime initialises.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

REPO = os.path.dirname(os.path.abspath(__file__))
for p in (REPO, os.path.join(REPO, "motion-latent-diffusion_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from mld_hip import _lib  # noqa: E402
from mld_hip import synthetic as syn  # noqa: E402

METRIC = "motions/sec (50-step DDIM + VAE decode), HumanML3D bs64, 1/2/4/8 GPU"      # BASELINE.json "metric", verbatim
FP32_MFMA_PEAK_TF = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32 dense peak
BF16_MFMA_PEAK_TF = 2500.0     # MI355X_MICROARCH.md: bf16 / f16 MFMA dense peak (no sparsity)
X3_PEAK_TF = BF16_MFMA_PEAK_TF / 3.0   # split-f16 kernels: three 16-bit MFMAs per algorithmic product
# The peaks above are quoted at the 2.4 GHz boost clock.  With matrix instructions issuing on (nearly) every CU the chip holds 1.87 GHz (measured with the loop's own cycle
# counter: 44.5 M cycles per wave in 18.8 ms on 160 CUs = 2.37 GHz, in 23.8 ms on 256 CUs = 1.87 GHz; profiles/r05_loop_experiments.json): every fraction of a chip-filling
# kernel is therefore also given against the peak at that sustained clock
SUSTAINED_CLOCK_RATIO = 1.87 / 2.4
BATCH, FRAMES, STEPS_DDIM = 64, 196, 50
PRECISIONS = {"f32": 0, "f16x3": 1, "bf16": 2}
PEAK_TF = {"f32": FP32_MFMA_PEAK_TF, "f16x3": X3_PEAK_TF, "bf16": BF16_MFMA_PEAK_TF}
DTYPE = {"f32": "f32 (exact-fp32 MFMA everywhere)",
         "f16x3": "split-f16: GEMM operands as hi + lo IEEE half, 3 x v_mfma_f32_16x16x32_f16 per product, fp32 accumulate (22 mantissa bits); "
                  "softmax / LayerNorm / residuals / scheduler fp32",
         "bf16": "bf16 MFMA operands in every GEMM, fp32 accumulate / attention / norms / residual stream"}
# profile-hook name -> (rocprofv3 kernel-name prefix, launches per sample()) at the two shapes the bench runs the loop at:
# one bs-64 request (6B = 384 rows: latency kernels, tile32.hpp) and coalesced requests (>= 768 rows: throughput kernels, strip.hpp)
KERNEL_LATENCY = {
    "den_qkv": ("void mld::gemm_tile32_kernel<32, 4, false", 9 * STEPS_DDIM),       # (<32,2> / <32,0> serve the layers after a skip linear / layer 0)
    "den_outproj": ("void mld::gemm_tile32_kernel<16, 0, false", 9 * STEPS_DDIM),
    "den_ffn1": ("void mld::gemm_tile32_kernel<32, 1, false", 9 * STEPS_DDIM),
    "den_ffn2": ("void mld::gemm_tile32_kernel<32, 0, false", 9 * STEPS_DDIM),
    "den_final": ("mld::den_final_step_kernel", STEPS_DDIM)}
KERNEL_THROUGHPUT = {   # strip.hpp template arguments: <slabs of src0, K segments, attention, PREC, ACT, column tiles per wave, waves>
    "den_qkv": ("void mld::gemm_strip_kernel<2, 1, false, 0, 0,", 9 * STEPS_DDIM),       # (<1,1,..> after a skip linear, <0,1,..> layer 0)
    "den_outproj": ("void mld::gemm_strip_kernel<0, 1, true, 0, 0,", 9 * STEPS_DDIM),
    "den_ffn1": ("void mld::gemm_strip_kernel<1, 1, false, 0, 1,", 9 * STEPS_DDIM),
    "den_ffn2": ("void mld::gemm_kernel<2, 2, 1, 2, false, true, 0, 16, false>", 9 * STEPS_DDIM),
    "den_final": ("mld::den_final_step_kernel", STEPS_DDIM)}
KERNEL_DECODE = {
    "dec_qkv": ("void mld::gemm_kernel<2, 4, 2, 2, false, true", 9), "dec_attn": ("void mld::attn_decode", 9),      # attn_decode_kernel (f32) / attn_decode_x3_kernel (the bf16-MFMA modes)
    "dec_outproj_ln": ("void mld::gemm_kernel<2, 4, 2, 4, true, true", 9), "dec_ffn1": ("void mld::gemm_kernel<2, 4, 2, 2, false, true", 9),
    "dec_ffn2_ln": ("void mld::gemm_kernel<2, 4, 2, 4, true, true", 9)}


KERNEL_DECODE_X3 = {   # split-bf16 modes: the feed-forward block is ONE launch (kernels/ffn_fused.hpp), the K = 256 staged GEMM serves QKV only
    "dec_qkv": KERNEL_DECODE["dec_qkv"], "dec_attn": KERNEL_DECODE["dec_attn"], "dec_outproj_ln": KERNEL_DECODE["dec_outproj_ln"],
    "dec_ffn": ("mld::ffn_x3_kernel", 9)}


def kernel_table(batch, precision="f16x3"):
    dec = KERNEL_DECODE_X3 if precision == "f16x3" else KERNEL_DECODE
    if dec is KERNEL_DECODE_X3 and batch * 4 >= 512:     # >= 512 (sample, head) pairs: the key-blocked attention kernel (mldhip.h "flash_attn")
        dec = {**dec, "dec_attn": ("void mld::attn_flash_x3_kernel<", 9)}
    return {**(KERNEL_THROUGHPUT if 6 * batch >= 768 else KERNEL_LATENCY), **dec}


def algorithmic_gflop(B, T, D=256, F=1024, L=9, NF=263, steps=STEPS_DDIM):
    """SURVEY.md App. C / BASELINE.md §5 (2*MAC GEMMs + 4*S*d attention; 1-key cross-attn shortcut)."""
    lin = lambda m, k, n: 2.0 * m * k * n
    m = 3 * 2 * B
    den = L * (lin(m, D, 3 * D) + lin(m, D, D) + 4.0 * m * 3 * D + lin(m, D, F) + lin(m, F, D)) + (L - 1) / 2 * lin(m, 2 * D, D)
    md = B * T
    dec = L * (lin(md, D, 3 * D) + lin(md, D, D) + 4.0 * md * T * D + lin(md, D, F) + lin(md, F, D) + 2 * lin(B, D, D)) \
        + (L - 1) / 2 * lin(md, 2 * D, D) + lin(md, D, NF)
    return (den * steps + dec) / 1e9, den / 1e9, dec / 1e9


class stdout_to_stderr:
    """File descriptor 1 points at stderr inside the block (C-level writers included: libc's buffers are flushed on both edges)."""

    def __enter__(self):
        sys.stdout.flush()
        C.CDLL(None).fflush(None)
        self.saved = os.dup(1)
        os.dup2(2, 1)

    def __exit__(self, *exc):
        sys.stdout.flush()
        C.CDLL(None).fflush(None)
        os.dup2(self.saved, 1)
        os.close(self.saved)


def source_hash():
    """Content hash of the engine sources (the GPU box has no .git): stamps profiles/*pmc* files so a stale one is refused."""
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(REPO, "motion-latent-diffusion_amd", "csrc", "**", "*.h*"), recursive=True)) \
        + [os.path.join(REPO, "include", "mldhip.h")]
    for f in files:
        h.update(os.path.relpath(f, REPO).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


LLVM_BIN = "/opt/rocm/lib/llvm/bin"


def mangled_part(kernel_name):
    """'void mld::den_loop_kernel<true, 4, 0, false>(mld::LoopArgs)' (a rocprofv3 kernel name) -> 'den_loop_kernelILb1ELi4ELi0ELb0EE':
    the piece of the Itanium-mangled symbol that identifies the instantiation (bool / int template arguments only)."""
    base, _, rest = kernel_name.partition("<")
    base = base.split("::")[-1].split()[-1]
    args = [a.strip() for a in rest.split(">")[0].split(",")] if rest else []
    enc = "".join("Lb%dE" % (a == "true") if a in ("true", "false") else "Li%sE" % a for a in args)
    return base + ("I" + enc + "E" if args else "")


def kernel_code_hash(name_part="den_loop_kernelILb1ELi4ELi0ELb0EE"):
    """Hash of the gfx950 MACHINE CODE of one kernel inside libmldhip.so (the persistent loop by default): the identity that ties a
    PMC summary to the build it is quoted for.  The whole-source hash above goes stale with any edit anywhere in csrc/; this one only
    when the compiled kernel itself changes.  None when the LLVM tools are missing."""
    tmp = tempfile.mkdtemp(prefix="mld_co_")
    try:
        fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "gfx950.co")
        subprocess.run([os.path.join(LLVM_BIN, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", _lib.DEFAULT_LIB, os.path.join(tmp, "copy.so")],
                       check=True, capture_output=True)
        subprocess.run([os.path.join(LLVM_BIN, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}", f"--output={co}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], check=True, capture_output=True)
        syms = subprocess.run([os.path.join(LLVM_BIN, "llvm-readelf"), "-s", "--wide", co], check=True, capture_output=True, text=True).stdout
        hits = {ln.split()[-1] for ln in syms.splitlines() if name_part in ln and " FUNC " in ln}      # (.dynsym and .symtab both list it)
        if len(hits) != 1:
            return None
        sym = hits.pop()
        dis = subprocess.run([os.path.join(LLVM_BIN, "llvm-objdump"), "-d", "--no-leading-addr", "--no-show-raw-insn", f"--disassemble-symbols={sym}", co],
                             check=True, capture_output=True, text=True).stdout
        body = [ln.split("//")[0].strip() for ln in dis.splitlines() if ln.startswith((" ", "\t"))]
        body = [ln for ln in body if ln]
        if len(body) < 100:
            return None
        return hashlib.sha256("\n".join(body).encode()).hexdigest()[:16]
    except Exception:
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def synthetic_state():
    t = {**{"denoiser." + k: v for k, v in syn.make_denoiser_state_dict().items()},
         **{"vae." + k: v for k, v in syn.make_vae_state_dict().items()}}
    t["mean"], t["std"] = syn.make_mean_std()
    return t


def pack_and_broadcast_weights(rank, dev):
    """Rank 0 builds the synthetic checkpoint; ONE broadcast ships it (RCCL over xGMI when world > 1)."""
    from mld_hip import dp
    template = synthetic_state()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    state = dp.broadcast_state(template if rank == 0 else {}, template, dev, src=0)
    torch.cuda.synchronize()
    return state, sum(v.size for v in template.values()) * 4, time.perf_counter() - t0


def device_identity(local):
    """(uuid or PCI bus id, name) of this rank's GPU -- all-gathered so the JSON proves N distinct devices took part."""
    pr = torch.cuda.get_device_properties(local)
    ident = getattr(pr, "uuid", None)
    if ident is None:
        ident = "pci:%s:%s:%s" % (getattr(pr, "pci_domain_id", "?"), getattr(pr, "pci_bus_id", "?"), getattr(pr, "pci_device_id", "?"))
    return str(ident), pr.name


def make_engine(local, weights, precision, max_batch=BATCH, nfl=1, graph=True, probe=True):
    eng = _lib.Engine(device=local, max_batch=max_batch, max_frames=FRAMES, use_graph=1 if graph else 0, precision=PRECISIONS[precision],
                      max_in_flight=nfl)
    eng.load_state_dict(weights)
    if not probe:
        eng.set_option("range_probe", 0)
    eng.finalize()
    return eng


def events_ms(stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    r = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), r


def rocprof_child_stats(precision, coalesce, extra=(), keep_env="MLD_BENCH_KEEP_ROCPROF", timeout=240):
    """rocprofv3 --kernel-trace --stats over a short single-stream run of THIS workload in a child process -> {kernel: (avg ns, calls, total ns)}."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found"
    out = tempfile.mkdtemp(prefix="mld_rocprof_")
    cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "bench", "--", sys.executable,
           os.path.abspath(__file__), "--profile-child", "--precision", precision, "--coalesce", str(coalesce)] + list(extra)
    try:
        subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), capture_output=True, text=True, timeout=timeout)
        files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return None, "no kernel_stats.csv produced"
        rows = list(csv.DictReader(open(files[0])))
        keep = os.environ.get(keep_env)     # tools/gpu_check.sh: keep the very summary the JSON line was computed from
        if keep:
            shutil.copy(files[0], keep)
        return {r["Name"]: (float(r["AverageNs"]), int(r["Calls"]), float(r["TotalDurationNs"])) for r in rows}, \
            "child run: bench.py --profile-child --coalesce %d %s(3 calls, one at a time)" % (coalesce, " ".join(extra) + " " if extra else "")
    except Exception as ex:  # never let the profiler take the bench down
        return None, repr(ex)[:200]
    finally:
        shutil.rmtree(out, ignore_errors=True)


def cpu_baseline(seed, threads, lengths_file=None, timeout=300, device="cpu", repeat=1):
    """The oracle ("port" of the reference path, torch-CPU backend) on the host cores: one full batch (64 motions, T=196,
    50 steps) in a child process with a bounded runtime.  Returns (info, joints)."""
    out_npy = "/tmp/mld_cpu_baseline_joints_%d.npy" % os.getpid()
    cmd = [sys.executable, os.path.join(REPO, "oracle", "cpu_baseline.py"), "--batch", str(BATCH), "--frames", str(FRAMES),
           "--seed", str(seed), "--threads", str(threads), "--out", out_npy, "--device", device, "--repeat", str(repeat)]
    if lengths_file:
        cmd += ["--lengths", lengths_file]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
        info = json.loads(r.stdout.strip().splitlines()[-1])
        return info, np.load(out_npy)
    except Exception as ex:  # timeout / parse failure: report it, never hang the bench
        return {"error": repr(ex)[:200]}, None


def run_steps(call, n, streams, single=None):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        call(i, single if single is not None else streams[i % len(streams)])
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def bench_a2m(local, dev, warmup, steps, streams, B=256, T=60):
    """BASELINE config 5 shape (config_mld_humanact12.yaml: action condition, 15-layer denoiser, ActorVae decoder, bs=256,
    T=60) in every arithmetic mode the library has (the fp8 denoiser mode BASELINE.json names was retired in round 6: see `retired_modes`), each with its measured error against
    the reference-generated fixture (tests/golden/action_b256.npz: final latents).  Secondary line, never `value`."""
    dims = syn.ModelDims(num_layers=15, nfeats=150)
    sdd, sdv = syn.make_denoiser_state_dict(seed=3, dims=dims, condition="action", nclasses=12), syn.make_actor_vae_state_dict()
    gold = np.load(os.path.join(REPO, "tests", "golden", "action_b256.npz"))
    acts, lat0, lens = syn.make_action_batch(B, nframes=T, seed=1234)      # the fixture's inputs (oracle/make_golden.py main_action)
    x0 = torch.from_numpy(lat0).to(dev)
    _, den15, _ = algorithmic_gflop(B, T, L=15, NF=150)
    _, _, dec6 = algorithmic_gflop(B, T, L=6, NF=150)
    gflop = den15 * STEPS_DDIM + dec6 - (6 - 1) / 2 * 2.0 * B * T * 512 * 256 / 1e9   # ActorVae has no skip linears
    modes, rejected = {}, {}
    nfl = len(streams)          # the caller's streams: their hardware-queue placement is already known to be good (DESIGN.md §3 point 15)
    for prec in ("f32", "f16x3", "bf16"):
        keep = prec in ("f32", "f16x3")      # bf16 fails every stated tolerance on these weights AND are slower than split-f16: reported under
                                             # `rejected_modes` (one bs-256 call at a time, with their error), not in the table of modes
        eng = _lib.Engine(device=local, max_batch=B, max_frames=T, condition=_lib.COND_ACTION, nclasses=12, vae_arch=_lib.VAE_ACTOR,
                          vae_num_layers=6, num_layers=15, nfeats=150, max_in_flight=nfl, precision=PRECISIONS[prec])
        eng.load_state_dict(sdd, "denoiser.")
        eng.load_state_dict(sdv, "vae.")
        eng.finalize()
        lat = torch.empty(B, 1, 256, device=dev)
        feats = [torch.empty(B, T, 150, device=dev) for _ in range(nfl)]
        eng.sample_action(acts, x0, lens, lat, feats[0])
        torch.cuda.synchronize()
        err = float(np.abs(lat.cpu().numpy() - gold["latents"]).max())
        call = lambda i, st: eng.sample_action(acts, x0, lens, None, feats[i % nfl], st.cuda_stream)
        run_steps(call, max(warmup, nfl), streams)
        dt = run_steps(call, steps, streams)
        n1 = max(2, steps // 2)
        dt1 = run_steps(call, n1, streams, single=streams[0]) / n1
        modes[prec] = {"value": round(B * steps / dt, 1), "value_single_batch": round(B / dt1, 1), "ms_per_step_single": round(dt1 * 1e3, 3),
                       "achieved_tflops": round(gflop / 1e3 / (dt / steps), 1), "max_abs_latents_vs_reference": err}
        modes[prec]["frac_of_mfma_peak"] = round(modes[prec]["achieved_tflops"] / (FP32_MFMA_PEAK_TF if prec in ("f32", "f16x3") else PEAK_TF[prec]), 4)
        modes[prec]["peak_note"] = "fp32 MFMA peak (the reverse loop, 90 % of this workload's FLOPs, runs exact fp32 on the column-split kernels at this batch)" \
            if prec in ("f32", "f16x3") else "dense 16-bit MFMA peak of the loop GEMMs' operand format"
        eng.close()
        if not keep:
            rejected[prec] = dict(modes.pop(prec), why="latents off by %.2g on |x| ~ 73 against the reference fixture (tolerance 5e-3): no parity claim; slower than f16x3 as well "
                                                       "(its GEMMs run on the round-2 column-split kernels, split-f16 on the persistent loop); the conclusion is about THESE random-init weights "
                                                       "under CFG 7.5 x 50 steps (profiles/r03_precision_ab.json), not about the format on trained weights" % err)
            continue
        # the engine-side way to keep the GPU full (no reliance on how streams land on hardware queues): four bs-256 requests in ONE
        # mldhip_sample_many call -- 1 024 motions: the f32 / f16x3 modes then run the sample-major persistent loop (15 layers)
        try:
            nreq = 4
            e4 = _lib.Engine(device=local, max_batch=nreq * B, max_frames=T, condition=_lib.COND_ACTION, nclasses=12, vae_arch=_lib.VAE_ACTOR,
                             vae_num_layers=6, num_layers=15, nfeats=150, max_in_flight=1, precision=PRECISIONS[prec])
            e4.load_state_dict(sdd, "denoiser.")
            e4.load_state_dict(sdv, "vae.")
            e4.finalize()
            reqs = []
            for i in range(nreq):
                a_i, l_i, n_i = (acts, lat0, lens) if i == 0 else syn.make_action_batch(B, nframes=T, seed=1234 + i)
                reqs.append(dict(actions=a_i, init_latents=torch.from_numpy(l_i).to(dev), lengths=n_i,
                                 latents_out=torch.empty(B, 1, 256, device=dev), feats_out=torch.empty(B, T, 150, device=dev)))
            e4.sample_many(reqs)
            torch.cuda.synchronize()
            err4 = float(np.abs(reqs[0]["latents_out"].cpu().numpy() - gold["latents"]).max())
            nrep = max(2, steps // nreq)
            t0 = time.perf_counter()
            for _ in range(nrep):
                e4.sample_many(reqs)
            torch.cuda.synchronize()
            dt4 = (time.perf_counter() - t0) / nrep
            modes[prec]["value_4_requests_per_call"] = round(nreq * B / dt4, 1)
            modes[prec]["max_abs_latents_vs_reference_4_requests_per_call"] = err4
            modes[prec]["launches_4_requests_per_call"] = list(e4.launch_counts())
            e4.close()
        except Exception as ex:      # noqa: BLE001 -- a secondary line must not take the bench down
            modes[prec]["value_4_requests_per_call"] = None
            modes[prec]["error_4_requests_per_call"] = repr(ex)[:200]
    return {"workload": "config_mld_humanact12.yaml (action-to-motion), bs=256, T=60, 50-step DDIM, CFG 7.5, ActorVae decode -> feats; "
                        "`value`: %d bs-256 calls in flight on %d streams (whether they overlap depends on how the streams land on hardware queues; "
                        "round 2's 8.6 k had that luck), reverse loop at 6B = 1536 rows on the throughput kernels (kernels/strip.hpp); "
                        "`value_4_requests_per_call`: four requests in ONE mldhip_sample_many call (1 024 motions)" % (nfl, nfl),
            "unit": "motions/s", "algorithmic_gflop_per_batch": round(gflop, 1),
            "latents_absmax": float(np.abs(gold["latents"]).max()), "reference_vs_oracle_floor_latents": float(gold["oracle_diff_latents"]),
            "modes": modes, "rejected_modes": rejected,
            "retired_modes": {"fp8_denoiser": "MLDHIP_PREC_FP8_DENOISER (ABI <= 4; BASELINE config 5 names fp8 MFMA denoiser GEMMs) was deleted in round 6 (VERDICT r5 item 7: faster than "
                                              "split-f16 or gone): its last measurement was latents off by 11.9 on |x| ~ 73 AND slower than f16x3 (BENCH_r05.json rejected_modes; "
                                              "profiles/r03_precision_ab.json: e4m3's 3-bit mantissa costs 2^-4 per operand whatever the scaling, amplified by guidance 7.5 x 50 steps)"}}


def bench_text_encoder(dev, n_texts=2 * BATCH, iters=10):
    """the frozen CLIP ViT-L/14 text tower is OUTSIDE the measured path (it stays on PyTorch-ROCm); this
    times a random-init tower of the same architecture (123.7 M parameters; no weights or tokenizer reachable offline) on the
    2B = 128 prompts of one bs-64 CFG batch, so the metric can also be read with text encoding included."""
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    cfg = CLIPTextConfig(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12, projection_dim=768,
                         vocab_size=49408, max_position_embeddings=77)
    model = CLIPTextModelWithProjection(cfg).eval().to(dev)
    ids = torch.randint(0, 49407, (n_texts, 77), device=dev)
    ids[:, -1] = 49407                                      # the EOS id the pooled output is read at
    with torch.no_grad():
        for _ in range(3):
            model(input_ids=ids)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            model(input_ids=ids)
        torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / iters * 1e3
    del model
    torch.cuda.empty_cache()
    return {"ms_per_128_prompts": round(ms, 3), "dtype": "f32", "weights": "random init (architecture of openai/clip-vit-large-patch14 text tower)",
            "backend": "PyTorch-ROCm (not part of libmldhip)"}


def bench_novae(local, dev, full, streams, B=64, T=196):
    """BASELINE config 4 shape (config_novae_humanml3d.yaml: raw-motion diffusion, trans_dec denoiser d=512, bs=64, T=196,
    DDPM).  The headline mode (f16x3) always runs the sampler's real 1000 steps (~5 s per pair of batches); the other
    two modes run 100 DDPM steps per batch (the same per-step work; their `value` is the EXTRAPOLATED 1000-step rate and says so)
    unless --novae-full-length.  Per arithmetic mode, `nfl` batches in flight on
    one handle (a workspace and a stream each)."""
    nfl = len(streams)
    steps = 1000 if full else 100
    b = syn.make_batch(B, None, seed=1234, max_len=T)
    text = torch.from_numpy(b.text_emb).to(dev)
    mean, std = syn.make_mean_std()
    weights = syn.make_novae_denoiser_state_dict()
    lin = lambda m, k, n: 2.0 * m * k * n
    m = 2 * B * T
    gf_step = (9 * (lin(m, 512, 1536) + 3 * lin(m, 512, 512) + 2 * lin(m, 512, 1024) + 4.0 * m * T * 512 + 4.0 * m * 2 * 512)
               + lin(m, 263, 512) + lin(m, 512, 263)) / 1e9
    # Two streams overlap only if ROCm put them on different hardware queues (it maps HIP streams onto 4 queues by reference count,
    # profiles/r02_hw_queue_placement.json): probe candidate pairs with a short run and keep the pair that overlaps best.
    placement = None
    if nfl == 2:
        probe = _lib.Engine(device=local, max_batch=B, max_frames=T, latent_dim=512, vae_arch=_lib.VAE_NONE, denoiser_arch=_lib.ARCH_TRANS_DEC,
                            scheduler_type=_lib.SCHED_DDPM, num_inference_steps=10, steps_offset=0, precision=PRECISIONS["f16x3"], max_in_flight=2)
        probe.load_state_dict(weights, "denoiser.")
        probe.load_tensor("mean", mean)
        probe.load_tensor("std", std)
        probe.finalize()
        px = [torch.randn(B, T, 263, device=dev) for _ in range(2)]
        pj = [torch.empty(B, T, 22, 3, device=dev) for _ in range(2)]
        cand = list(streams) + [torch.cuda.Stream(device=dev) for _ in range(3)]
        placement = {}
        for j in range(1, len(cand)):
            ts = []
            for rep in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i, st in enumerate((cand[0], cand[j])):
                    probe.sample_novae(text, px[i], b.lengths, None, 7 + i, None, pj[i], st.cuda_stream)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            placement["0+%d" % j] = round(min(ts[1:]) * 1e3 / 20, 3)          # ms per DDPM step and batch (first repetition: graph capture)
        best = min(placement, key=placement.get)
        streams = [cand[0], cand[int(best.split("+")[1])]]
        placement = {"ms_per_ddpm_step_by_stream_pair_10_step_probe": placement, "picked": best}
        probe.close()
    modes = {}
    for prec in ("f32", "f16x3", "bf16"):
        steps = 1000 if (full or prec == "f16x3") else 100
        # ONE handle, `nfl` workspaces (max_in_flight), one stream per batch, calls issued from this thread one after another (they return once
        # their step graphs are enqueued): the batches share the weight images in L2 / Infinity Cache.  (Rounds 2-4 used a handle + host thread
        # per batch: 5.99 against 5.08 ms per DDPM step and batch in the split mode, r04 -- tools/ab_novae_gemm.py measures this form.)
        eng = _lib.Engine(device=local, max_batch=B, max_frames=T, latent_dim=512, vae_arch=_lib.VAE_NONE, denoiser_arch=_lib.ARCH_TRANS_DEC,
                          scheduler_type=_lib.SCHED_DDPM, num_inference_steps=steps, steps_offset=0, precision=PRECISIONS[prec], max_in_flight=nfl)
        eng.load_state_dict(weights, "denoiser.")
        eng.load_tensor("mean", mean)
        eng.load_tensor("std", std)
        eng.finalize()
        x0 = [torch.randn(B, T, 263, device=dev) for _ in range(nfl)]
        joints = [torch.empty(B, T, 22, 3, device=dev) for _ in range(nfl)]
        torch.cuda.synchronize()

        def run(seed0):
            t0 = time.perf_counter()
            for i in range(nfl):
                eng.sample_novae(text, x0[i], b.lengths, None, seed0 + i, None, joints[i], streams[i].cuda_stream)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        run(99)                              # untimed: captures each handle's step-chunk graphs
        dt = run(1234)
        ms_step = dt * 1e3 / (steps * nfl)
        ms_step2 = None
        if prec == "f16x3" and placement is not None:
            # the 10-step probe above is a burst on a cool chip; the mode's figure is seconds of sustained matrix work.  A second full-length run on the SAME pair of
            # streams says whether the first was a placement accident (it would differ) or the clock the chip holds (it repeats)
            ms_step2 = run(4321) * 1e3 / (steps * nfl)
            placement["ms_per_ddpm_step_second_full_run"] = round(ms_step2, 3)
            placement["note"] = ("probe = 2 batches x 10 steps on a cool chip (a burst: boost clock); ms_per_ddpm_step of the mode = all %d steps of %d batches, ~%.0f s of sustained "
                                 "matrix work on every CU (the chip holds ~1.9 GHz there, not ~2.4: MI355X_MICROARCH.md DVFS) -- the probe picks the stream pair, it is not the rate; "
                                 "round 5 quoted the two side by side as if they measured the same thing" % (steps, nfl, dt))
        modes[prec] = {"ms_per_ddpm_step": round(ms_step, 3), "achieved_tflops": round(gf_step / ms_step, 1),
                       "frac_of_mfma_peak": round(gf_step / ms_step / PEAK_TF[prec], 4), "peak_tflops_of_this_mode": round(PEAK_TF[prec], 1),
                       "value": round(B / ms_step, 3), "finite": bool(all(torch.isfinite(j).all().item() for j in joints)),
                       "ddpm_steps_run": steps, "seconds_for_the_timed_batches": round(dt, 3), "extrapolated_from_steps": None if steps == 1000 else steps}
        eng.close()
    return {"workload": "config_novae_humanml3d.yaml (raw-motion diffusion, trans_dec d=512), bs=64, T=196, DDPM, CFG 7.5 -> joints; "
                        "%d batches in flight on one handle (one stream each); f16x3: all 1000 DDPM steps run per batch, other modes %d" % (nfl, 1000 if full else 100),
            "unit": "motions/s of the 1000-step sampler (= 64 / (1000 x ms_per_ddpm_step))", "extrapolated_from_steps": "per mode: see modes[*].extrapolated_from_steps (f16x3: none)",
            "algorithmic_gflop_per_ddpm_step": round(gf_step, 1), "kernel_launches_per_ddpm_step": 78,
            "cross_fold": "round 6: LayerNorm 1 + the two-token cross-attention sub-layer + LayerNorm 2 of every layer are ONE launch on vectors folded from the memory tokens (exact algebra; "
                          "no query GEMM, no out-projection GEMM: 26 of a step's 1 290 algorithmic GFLOP are not executed as products any more -- the fractions above still divide the reference's count by the time)", "modes": modes, "stream_placement": placement,
            "error_vs_reference": "f32: tests/test_gpu_parity.py::test_novae_full_length_1000_steps_vs_reference_golden; every mode: "
                                  "tools/ab_precision.py -> profiles/r03_precision_ab.json",
            "peaks": "f32: fp32 MFMA 157.3 TF; f16x3: dense 16-bit MFMA peak / 3 (three MFMAs per product) = 833 TF; bf16: 2500 TF"}


PMC_FILE = next((f for f in (os.path.join(REPO, "profiles", "r06_pmc_traffic.json"), os.path.join(REPO, "profiles", "r05_pmc_traffic.json")) if os.path.exists(f)),
                os.path.join(REPO, "profiles", "r06_pmc_traffic.json"))


def pmc_summary(coalesce, loop_code_hash):
    """The PMC summary (tools/gpu_pmc.sh: separate rocprofv3 --pmc passes) of THIS call shape: profiles/r05_pmc_traffic.json holds one
    entry per requests-per-call it was collected at (1 = one bs-64 request: the cluster loop, 20 = the driver's `--steps 20`, 32 = the chip-filling call).  Refused when it was
    collected on other machine code of the loop kernel AND on other sources."""
    try:
        pmc = json.load(open(PMC_FILE))
    except Exception:
        return None, "no PMC summary (%s)" % os.path.relpath(PMC_FILE, REPO)
    ent = pmc.get("shapes", {}).get(str(coalesce))
    if ent is None:
        return None, "%s has no entry for %d requests per call (has: %s)" % (os.path.relpath(PMC_FILE, REPO), coalesce, sorted(pmc.get("shapes", {})))
    same_code = loop_code_hash is not None and ent.get("loop_kernel_code_hash") == loop_code_hash
    if not (same_code or ent.get("source_hash") == source_hash()):
        return None, "%s[%d] was collected on kernel code %s / source hash %s, this run is %s / %s: refused as stale" % (
            os.path.relpath(PMC_FILE, REPO), coalesce, ent.get("loop_kernel_code_hash"), ent.get("source_hash"), loop_code_hash, source_hash())
    return ent, ("%s[%d requests per call]: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes on THIS %s and call shape; L2<->fabric bytes per launch"
                 % (os.path.relpath(PMC_FILE, REPO), coalesce, "machine code of the loop kernel (%s)" % loop_code_hash if same_code else "source hash"))


# decoder kernels of the split-f16 mode at chip-filling launches: rocprofv3 name prefix, launches per call, algorithmic HBM bytes and
# FLOPs per frame row (fp32 activations, 256 wide: 1 KB per row and tensor) -- DESIGN.md section 3's per-kernel table, computed live
HBM_PEAK_TBS, HBM_COPY_TBS = 8.0, 6.3            # MI355X_MICROARCH.md: spec peak / measured float4 copy
DECODER_KERNELS = {
    "in_projection": ("void mld::strip_gemm_x3_kernel<6, 1, false, true", 8, (256 + 768) * 4, 2.0 * 256 * 768, "dec_qkv",
                      "row strip in (1 KB / row), packed Q|K|V out (3 KB / row): write-heavy stream"),
    "self_attention": ("mld::attn_flash_x3_kernel", 9, (768 + 256) * 4, None, "dec_attn",
                       "key-blocked online softmax over T = 196: Q|K|V in, attention output out; 4 T 256 FLOP per row"),
    "decoder_tail": ("void mld::ffn_strip_x3_kernel<3, true", 9, 3 * 256 * 4, 2.0 * (256 * 256 + 2 * 256 * 1024), "dec_ffn",
                     "out-projection + norms + feed-forward block: attention output + residual in, layer output out"),
    "skip_linear": ("void mld::strip_gemm_x3_kernel<4, 2, false, false", 4, 3 * 256 * 4, 2.0 * 512 * 256, "dec_skip",
                    "Linear(cat[x, skip]): two row strips in, one out"),
    "final_norm_linear": ("mld::final_strip_x3_kernel", 1, (256 + 263) * 4, 2.0 * 256 * 263, None,
                          "decoder.norm + final_layer (N = 263) + padded-frame zeroing as one row-strip launch"),
}


def decoder_roofline(stats, motions, pmc_shape):
    """Per decoder kernel of the headline call: algorithmic HBM bytes and FLOPs per launch / the rocprofv3 dispatch average of the SAME
    child run the loop's roofline uses -> TB/s against the 8 TB/s spec and the 6.3 TB/s a copy reaches, TFLOP/s against the split-f16
    MFMA roof; measured traffic and MFMA-busy from the PMC summary of this shape when there is one."""
    if not stats:
        return {"error": "no rocprofv3 kernel stats"}
    M = motions * FRAMES
    out = {"rows_per_launch": M, "unit": "TB/s | TFLOP/s", "hbm_peak_tb_s": HBM_PEAK_TBS, "hbm_copy_tb_s": HBM_COPY_TBS, "mfma_roof_tflops": round(X3_PEAK_TF, 1), "kernels": {}}
    tot_ms = 0.0
    for name, (prefix, per_call, bytes_row, flop_row, pmc_key, what) in DECODER_KERNELS.items():
        hits = [(n, v) for n, v in stats.items() if n.startswith(prefix)]
        if not hits:
            continue
        n, (avg, calls_, total) = max(hits, key=lambda kv: kv[1][2])
        rows = M if name != "in_projection" else M        # (layer 0 projects ONE sample's rows: a tiny ninth launch, not in this average's class)
        gb = bytes_row * rows / 1e9
        fl = (flop_row if flop_row is not None else 4.0 * FRAMES * 256) * rows
        ent = {"kernel": n[:90], "launches_per_call": per_call, "avg_us": round(avg / 1e3, 1), "algorithmic_gb_per_launch": round(gb, 3),
               "tb_s": round(gb / (avg * 1e-9) / 1e3, 3), "frac_of_8_tb_s": round(gb / (avg * 1e-9) / 1e3 / HBM_PEAK_TBS, 3),
               "frac_of_copy_rate": round(gb / (avg * 1e-9) / 1e3 / HBM_COPY_TBS, 3), "tflops": round(fl / (avg * 1e-9) / 1e12, 1),
               "frac_of_mfma_roof": round(fl / (avg * 1e-9) / 1e12 / X3_PEAK_TF, 3), "what": what}
        ent["bound"] = "hbm" if ent["frac_of_copy_rate"] >= ent["frac_of_mfma_roof"] else "mfma"
        k = (pmc_shape or {}).get("kernels", {}).get(pmc_key) if pmc_key else None
        if k and "traffic_bytes_per_launch" in k:
            ent["traffic_gb_per_launch_pmc"] = round(k["traffic_bytes_per_launch"] / 1e9, 3)
        sq = (pmc_shape or {}).get("sq", {}).get(pmc_key) if pmc_key else None
        if sq:
            ent.update({kk: sq[kk] for kk in ("mfma_busy_frac", "valu_per_mfma") if kk in sq})
        tot_ms += avg * per_call / 1e6
        out["kernels"][name] = ent
    out["decode_ms_per_call_sum_of_these"] = round(tot_ms, 2)
    return out


def make_requests(dev, n, rank, with_lat=False):
    """n bs-64 requests, each with its own prompts / noise (seeded per rank and slot) and output buffers, all resident in HBM"""
    reqs = []
    for sl in range(n):
        bt = syn.make_batch(BATCH, None, seed=1234 + rank + 1000 * sl, max_len=FRAMES)
        r = dict(text_emb=torch.from_numpy(bt.text_emb).to(dev), init_latents=torch.from_numpy(bt.init_latents).to(dev), lengths=bt.lengths,
                 joints_out=torch.empty(BATCH, FRAMES, 22, 3, device=dev))
        if with_lat:
            r["latents_out"] = torch.empty(BATCH, 1, 256, device=dev)
        reqs.append(r)
    return reqs


def profile_child(a):
    """--profile-child: the headline call shape (a.coalesce bs-64 requests per mldhip_sample_many call; 1 = a plain mldhip_sample),
    one call at a time, a few calls; run under rocprofv3 by rocprof_child_stats() and tools/gpu_pmc.sh."""
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    c = max(1, a.coalesce)
    # (no range probe here: finalize's probe launches the loop kernel for two reverse steps, a ~1 ms dispatch of the SAME kernel name that
    #  would sit in rocprofv3's per-kernel average and in the PMC per-dispatch means; the timed engine of main() runs it -- `numeric` in the line)
    eng = make_engine(0, synthetic_state(), a.precision, max_batch=BATCH * c, probe=False)
    for kv in filter(None, os.environ.get("MLD_BENCH_SET", "").split(",")):      # per-handle options for A/B profiles: "attn_tr=0,nt_hints=0"
        k, v = kv.split("=")
        eng.set_option(k, int(v))
    reqs = make_requests(dev, c, 0)
    for _ in range(max(1, a.steps if a.steps < 20 else 3)):
        if c == 1:
            eng.sample(reqs[0]["text_emb"], reqs[0]["init_latents"], reqs[0]["lengths"], None, None, reqs[0]["joints_out"])
        else:
            eng.sample_many(reqs)
    torch.cuda.synchronize()


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(dirname, arrays):
    """--dump-outputs: {name: array} -> dirname/<name>.npy in float32, refused above DUMP_LIMIT_BYTES in all."""
    arrays = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in arrays.items()}
    total = sum(v.nbytes for v in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise ValueError("--dump-outputs: %d bytes exceed the %d-byte limit" % (total, DUMP_LIMIT_BYTES))
    os.makedirs(dirname, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(dirname, k + ".npy"), v)
    return total


def spread(ts):
    ts = sorted(ts)
    return {"median": ts[len(ts) // 2], "min": ts[0], "max": ts[-1], "n": len(ts)}


def emit(out):
    """The whole evidence blob (every table, ~20 KB) goes to a FILE ($MLD_BENCH_EVIDENCE, default ./bench_evidence.json; also to stderr as one `EVIDENCE {...}` line) and the
    contract's ONE stdout line stays under 8 KB: round 5's line was cut off by the driver's tail and its parser dropped the top-level keys it does not know (VERDICT r5
    weak #8 / item 6) -- the literal-configuration numbers now live inside `config`, the single-batch roofline inside `roofline`."""
    blob = json.dumps(out)
    path = os.environ.get("MLD_BENCH_EVIDENCE", os.path.join(os.getcwd(), "bench_evidence.json"))
    try:
        with open(path, "w") as f:
            f.write(blob + "\n")
    except OSError as ex_:
        path = "unwritable: %r" % (ex_,)
    print("EVIDENCE " + blob, file=sys.stderr, flush=True)
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "repeats", "config")
    line = {k: out[k] for k in keep if k in out}
    pick = lambda d, ks: {k: d[k] for k in ks if isinstance(d, dict) and k in d}
    r = out.get("roofline") or {}
    line["roofline"] = pick(r, ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "shape", "frac_hip_events", "peak_at_sustained_clock", "frac_at_sustained_clock",
                                "frac_on_occupied_cus", "workgroups", "gflop_per_launch", "avg_us_rocprof_dispatch", "algorithmic_bytes_per_launch", "source_hash",
                                "loop_kernel_code_hash", "rocprof"))
    sb = out.get("single_batch") or {}
    if sb:
        line["roofline"]["single_batch"] = dict(pick(sb, ("value", "unit", "ms_per_batch", "launches_per_call")),
                                                roofline=pick(sb.get("roofline") or {}, ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "workgroups",
                                                                                         "avg_us_rocprof_dispatch", "l2_to_cu_fill", "kernel_code_hash")))
        lf = line["roofline"]["single_batch"]["roofline"].get("l2_to_cu_fill")
        if isinstance(lf, dict):
            line["roofline"]["single_batch"]["roofline"]["l2_to_cu_fill"] = pick(lf, ("weight_bytes_per_member_and_launch", "achieved_frac_of_56_B_per_clk_per_cu"))
    if out.get("bs64_pipelined"):
        line["roofline"]["bs64_pipelined"] = pick(out["bs64_pipelined"], ("value", "unit", "ms_per_request", "requests_per_call", "numeric", "error"))
    dr = out.get("decoder_roofline") or {}
    if isinstance(dr, dict):
        line["decoder"] = {k: v for k, v in dr.items() if not isinstance(v, (dict, list))}
    line["cpu_baseline"] = pick(out.get("cpu_baseline") or {}, ("value", "unit", "cores", "kind", "sample", "host_cpus"))
    line["parity"] = pick(out.get("parity") or {}, ("tolerance", "motions_checked", "max_abs_joints_vs_exact_fp32_engine_all_requests", "max_abs_joints_vs_oracle",
                                                    "max_abs_joints_vs_oracle_single_call"))
    line["numeric"] = pick((out.get("numeric") or {}), ("range_probe", "nonfinite_values_in_timed_calls"))
    line["eager_same_gpu"] = pick(out.get("eager_same_gpu") or {}, ("value", "unit"))
    ow = []
    for w in out.get("other_workloads") or []:
        m = (w.get("modes") or {}).get("f16x3") or {}
        ow.append({"workload": str(w.get("workload", ""))[:70], "f16x3": pick(m, ("value", "ms_per_ddpm_step", "frac_of_mfma_peak", "ddpm_steps_run", "max_abs_latents_vs_golden",
                                                                                "value_single_batch"))})
    line["other_workloads"] = ow
    line["distributed"] = pick(out.get("distributed") or {}, ("backend", "world_size", "distinct_devices", "data_path_collectives"))
    line = {k: v for k, v in line.items() if v != {} and v != []}        # (a plain run measures the headline only: no rooflines, baselines or other workloads)
    line["evidence"] = {"file": path, "bytes": len(blob), "note": "every table of this run (kernels, decoder_roofline, sweeps, alt modes, other workloads in full): the file, and the EVIDENCE line on stderr"}
    text = json.dumps(line)
    if len(text) > 8000:                       # never: but the contract is one parseable line the driver's tail keeps whole
        for k in ("other_workloads", "decoder", "eager_same_gpu", "numeric"):
            line.pop(k, None)
        text = json.dumps(line)
    print(text, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--precision", choices=list(PRECISIONS)[:3], default=os.environ.get("MLD_BENCH_PRECISION", "f16x3"),
                    help="arithmetic mode of the headline (see the module docstring); the others are reported as alt_modes")
    ap.add_argument("--coalesce", type=int, default=int(os.environ.get("MLD_BENCH_COALESCE", "32")),
                    help="bs-64 requests per engine call (mldhip_sample_many), at most 32; 1 = one call per request")
    ap.add_argument("--repeats", type=int, default=None,
                    help="repetitions of the K-step timed region (median reported, min / max carried); default 1, 5 with --full")
    ap.add_argument("--eager", action="store_true", help="disable hipGraph replay (debug)")
    ap.add_argument("--full", action="store_true",
                    help="also run every secondary measurement (single-batch / pipelined figures, rooflines, sweep, CPU baseline, parity, other modes and workloads)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's outputs (latents, joints) to DIR/<name>.npy, float32")
    ap.add_argument("--novae-full-length", action="store_true", help="with --full: run the config-4 leg at its real length in every mode (1000 DDPM steps; ~1 min)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-rocprof", action="store_true", help="skip the rocprofv3 children (rooflines fall back to HIP events)")
    ap.add_argument("--no-alt", action="store_true", help="skip the alternate arithmetic modes and serving shapes")
    ap.add_argument("--no-a2m", action="store_true", help="skip the secondary action-to-motion (config 5) measurement")
    ap.add_argument("--no-clip", action="store_true", help="skip timing a random-init CLIP text tower on PyTorch-ROCm")
    ap.add_argument("--no-novae", action="store_true", help="skip the secondary diffusion-only (config 4) measurement")
    ap.add_argument("--profile-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.profile_child:
        return profile_child(a)
    if a.repeats is None:
        a.repeats = 5 if a.full else 1

    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: become the launcher -- one rank per GPU under torch.distributed.run, same flags
        import socket
        assert torch.cuda.is_available(), "bench.py needs an MI355X (no CPU path)"
        have = torch.cuda.device_count()
        if have < a.gpus:
            sys.exit(f"bench.py: --gpus {a.gpus} but only {have} GPU(s) are visible")
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.run(cmd, env=env).returncode)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        sys.exit(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={world} (launch with --nproc-per-node {a.gpus}, or without torchrun)")
    assert torch.cuda.is_available(), "bench.py needs an MI355X (no CPU path)"
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = None
    if world > 1 or "WORLD_SIZE" in os.environ:      # under torchrun the collective path runs at every world size, 1 included
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        with stdout_to_stderr():                     # RCCL prints its version banner on stdout when the communicator comes up: rank 0's stdout is ONE JSON line
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
            dist.barrier()
            torch.cuda.synchronize()

    K = a.steps
    coalesce = max(1, min(32, a.coalesce, K))
    weights, weight_bytes, bcast_s = pack_and_broadcast_weights(rank, dev)
    MAXC = 32                                    # the engine is sized for the chip-filling call (2 048 motions) whatever K is: the sweep below uses it
    eng = make_engine(local, weights, a.precision, max_batch=BATCH * MAXC, graph=not a.eager)
    ident = (rank, local) + device_identity(local)
    ranks_seen = [ident]
    if dist:
        ranks_seen = [None] * world
        dist.all_gather_object(ranks_seen, ident)
    stream = torch.cuda.current_stream()
    reqs_all = make_requests(dev, MAXC if a.full else coalesce, rank, with_lat=True)     # (seeded per slot: the first `coalesce` are the same either way)
    reqs = reqs_all[:coalesce]
    calls = [coalesce] * (K // coalesce) + ([K % coalesce] if K % coalesce else [])     # requests per call of one timed region: exactly K steps
    warm = sorted(set(calls), reverse=True)      # warm-up: every call shape of the timed region once (its graph is captured), then W steps in all at least
    while sum(warm) < a.warmup:
        warm.append(calls[0])

    def issue(e_, lengths=None, shape=None):
        for n in shape or calls:
            if n == 1:
                r = reqs[0]
                e_.sample(r["text_emb"], r["init_latents"], lengths[0] if lengths else r["lengths"], r["latents_out"], None, r["joints_out"], stream.cuda_stream)
            else:
                e_.sample_many([dict(r, lengths=lengths[i]) if lengths else r for i, r in enumerate(reqs[:n])], stream.cuda_stream)

    def issue_single(e_, nsteps):
        for i in range(nsteps):
            r = reqs[i % len(reqs)]
            e_.sample(r["text_emb"], r["init_latents"], r["lengths"], r["latents_out"], None, r["joints_out"], stream.cuda_stream)

    def timed(fn):
        torch.cuda.synchronize()
        if dist:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        own = time.perf_counter() - t0           # this rank's own K steps (before waiting for the slowest rank)
        if dist:
            dist.barrier()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        per_rank = [own]
        if dist:
            t = torch.tensor([dt], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
            g = [torch.zeros(1, device=dev, dtype=torch.float64) for _ in range(world)]
            dist.all_gather(g, torch.tensor([own], device=dev, dtype=torch.float64))
            per_rank = [float(x.item()) for x in g]
        return dt, per_rank

    torch.cuda.synchronize()                     # inputs were uploaded on the default stream
    issue(eng, shape=warm)
    launches_headline = eng.launch_counts()      # [reverse loop, decode, joints] launches of the last (headline-shaped) call
    numeric0 = eng.numeric_status()              # what finalize's range probe decided (mldhip.h "Range contract")
    if a.full:
        issue_single(eng, 2)
        launches_single = eng.launch_counts()    # ... of a single bs-64 call
    reps = [timed(lambda: issue(eng)) for _ in range(max(1, a.repeats))]
    order = sorted(range(len(reps)), key=lambda i: reps[i][0])
    dt, per_rank_s = reps[order[len(order) // 2]]            # the median repetition IS the reported K-step region
    ms_per_step = dt / K * 1e3
    value = world * BATCH * K / dt
    if a.dump_outputs and rank == 0:
        last = reqs[calls[-1] - 1]               # the last timed step = the last request of the last call (its buffers are not touched again before this)
        dump_outputs(a.dump_outputs, {"latents": last["latents_out"].cpu().numpy(), "joints": last["joints_out"].cpu().numpy()})
    if a.full:                                   # the single-batch and pipelined figures
        K1 = min(K, 16)
        reps1 = [timed(lambda: issue_single(eng, K1))[0] / K1 for _ in range(max(1, a.repeats))]     # strictly one bs-64 batch after another
        ms1 = spread(reps1)
        # ---- bs-64 requests back to back with the two halves of consecutive requests overlapped ("many_pipeline": decode of request k on the engine's side stream beside the
        #      cluster launch of request k + 1; every request bit-identical to its serial mldhip_sample call -- tests/test_gpu_parity.py).  K steps per timed region, as above.
        pipe = None
        try:
            engp = make_engine(local, weights, a.precision, max_batch=BATCH, nfl=2, graph=not a.eager)
            engp.set_option("many_pipeline", 1)
            KP = min(K, 32)
            pcalls = [KP] * (K // KP) + ([K % KP] if K % KP else [])

            def issue_pipe():
                for n in pcalls:
                    if n == 1:
                        r = reqs_all[0]
                        engp.sample(r["text_emb"], r["init_latents"], r["lengths"], r["latents_out"], None, r["joints_out"], stream.cuda_stream)
                    else:
                        engp.sample_many(reqs_all[:n], stream.cuda_stream)
            issue_pipe(); issue_pipe()
            repsp = [timed(issue_pipe)[0] / K for _ in range(max(1, a.repeats))]
            msp = spread(repsp)
            nsp = engp.numeric_status()
            pipe = {"value": round(world * BATCH / msp["median"], 2), "unit": "motions/s", "ms_per_request": {k: (round(v * 1e3, 4) if k != "n" else v) for k, v in msp.items()},
                    "requests_per_call": KP, "numeric": {k: nsp[k] for k in ("nonfinite_values", "cluster_loop")},
                    "shape": "mldhip_sample_many with option many_pipeline = 1: %d bs-64 requests per call, one after the other on the single-request path (cluster loop), decode of "
                             "request k on the engine's low-priority side stream beside the reverse loop of request k + 1; two workspaces alternate; the caller's stream is ordered "
                             "behind every decode at the end of the call" % KP}
            engp.close()
        except Exception as ex_:      # never fail the single-process bench line for the secondary leg
            if dist:                  # ... but under torch.distributed a rank that skipped its barriers would hang the others: fail loudly instead
                raise
            pipe = {"value": None, "error": repr(ex_)[:300]}
    gf_total, gf_den, gf_dec = algorithmic_gflop(BATCH, FRAMES)
    tf_job = gf_total / 1e3 / (ms_per_step * 1e-3)
    PB = BATCH * coalesce

    out = {
        "metric": METRIC, "value": round(value, 2), "unit": "motions/s", "n_gpus": world, "steps": K, "warmup": a.warmup,
        "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": DTYPE[a.precision], "data": "synthetic",
        "repeats": {"n": len(reps), "value_median": round(value, 2), "value_min": round(world * BATCH * K / max(r[0] for r in reps), 2),
                    "value_max": round(world * BATCH * K / min(r[0] for r in reps), 2),
                    "note": "the K-step timed region repeated n times, barrier + synchronize on both sides of each; `value` / `ms_per_step` are the median repetition"},
        "config": {"workload": "config_mld_humanml3d.yaml, bs=64 per step (request), T=196, 50-step DDIM, CFG 7.5, VAE decode + feats2joints; "
                               "%d requests (%d motions) per engine call (mldhip_sample_many: the reverse loop of a call is ONE persistent launch, "
                               "a workgroup per 8 motions), calls one after another on one stream; `single_batch`: one bs-64 batch at a time" % (coalesce, PB),
                   "requests_per_call": coalesce, "calls_per_timed_region": len(calls), "in_flight": 1, "global_batch": PB * world, "batch_per_request": BATCH,
                   "parallelism": f"dp{world}", "graph": not a.eager, "precision": a.precision,
                   "weights": "synthetic (seeded numpy), one broadcast of %.1f MB" % (weight_bytes / 1e6),
                   "launches_per_call": launches_headline},
        "whole_job": {"algorithmic_gflop_per_batch": round(gf_total, 1), "denoise_gflop_per_step": round(gf_den, 3), "decode_gflop": round(gf_dec, 1),
                      "achieved_tflops": round(tf_job, 2), "frac_of_fp32_mfma_peak": round(tf_job / FP32_MFMA_PEAK_TF, 4),
                      "frac_of_mode_peak": round(tf_job / PEAK_TF[a.precision], 4), "mode_peak_tflops": round(PEAK_TF[a.precision], 1),
                      "note": "per GPU; mode peak = the MFMA roof of the headline arithmetic (f16x3: dense f16 peak / 3 products)"},
    }
    if a.full:
        out["config"].update({
                   # the configuration BASELINE.json's metric is quoted on, inside `config` so that a parser that keeps only the contract's keys keeps it
                   "value_single_batch": round(world * BATCH / ms1["median"], 2), "ms_single_batch": round(ms1["median"] * 1e3, 4),
                   "value_bs64_pipelined": pipe.get("value") if pipe else None,
                   "ms_per_request_bs64_pipelined": (pipe.get("ms_per_request") or {}).get("median") if pipe else None,
                   "single_batch_note": "value_single_batch: ONE bs-64 mldhip_sample call at a time, strictly serial (the metric's literal configuration); value_bs64_pipelined: the same "
                                        "bs-64 requests back to back with decode(k) beside loop(k + 1) (many_pipeline); value: the serving shape, requests_per_call requests as one chain"})
    ns = eng.numeric_status()
    out["numeric"] = {"range_probe": numeric0, "nonfinite_values_in_timed_calls": ns["nonfinite_values"],
                      "note": "F16X3 range contract: probe at finalize (split-f16 vs exact-fp32 kernels of the same handle), fp32 fallback per stage above MLDHIP_PROBE_TOL = %g, "
                              "non-finite latents / joints counted at run time" % _lib.PROBE_TOL}
    per_rank_v = [BATCH * K / t for t in per_rank_s]
    out["distributed"] = {"backend": "nccl (RCCL)" if dist else "none (single process)", "world_size": world,
                          "ranks_seen": [list(r) for r in ranks_seen], "distinct_devices": len({r[2] for r in ranks_seen}),
                          "weight_broadcast": {"bytes": weight_bytes, "seconds": round(bcast_s, 4), "collectives": 1 if dist else 0,
                                               "note": "one packed broadcast from rank 0 (includes host->device staging on rank 0)"},
                          "per_rank_motions_per_s": {"min": round(min(per_rank_v), 2), "max": round(max(per_rank_v), 2)},
                          "data_path_collectives": 0}
    if rank == 0 and a.full:
        solo = world == 1 and not a.eager
        # ---- headline call shape under rocprofv3 (child process, same call shape, one call at a time): per-kernel table + the dominant kernel
        stats, where = (None, "disabled") if (a.no_rocprof or dist is not None or a.eager) else rocprof_child_stats(a.precision, coalesce)
        # HIP events on the launch stream around loop-only calls (latents out, no decode): the persistent loop kernel + the condition-row GEMM
        lat_only = [dict(text_emb=r["text_emb"], init_latents=r["init_latents"], lengths=r["lengths"], latents_out=r["latents_out"]) for r in reqs]
        if coalesce > 1:
            eng.sample_many(lat_only, stream.cuda_stream)
            loop_ms = min(events_ms(stream, lambda: eng.sample_many(lat_only, stream.cuda_stream))[0] for _ in range(3))
        else:
            loop_ms = None
        fused = launches_headline[0] <= 4
        x3 = a.precision == "f16x3"
        flop_loop_call = gf_den * STEPS_DDIM * coalesce          # GFLOP of one call's reverse loop
        kern = {}
        if stats:
            tot = sum(v[2] for v in stats.values()) or 1.0
            for n, (avg, calls_, total) in sorted(stats.items(), key=lambda kv: -kv[1][2])[:12]:
                kern[n[:110]] = {"avg_us": round(avg / 1e3, 2), "calls": calls_, "share_of_gpu_time": round(total / tot, 4)}
        roof = {"bound": "mfma", "unit": "TFLOP/s", "source_hash": source_hash(),
                "shape": "one headline call: %d motions, decoder at %d frame rows" % (PB, PB * FRAMES),
                "rocprof": where if stats else "unavailable: %s" % where}
        loop_rows = [(n, v) for n, v in (stats or {}).items() if "den_loop_kernel" in n]
        if fused and (loop_rows or loop_ms):
            avg_us = loop_rows[0][1][0] / 1e3 if loop_rows else None
            # the live measurement: HIP events on the launch stream around loop-only calls of THIS process (the persistent launch + the 20-us
            # condition-row GEMM + the latent copies); the rocprofv3 dispatch average of the child run is carried beside it -- under the
            # profiler the same kernel runs 5-10 % slower (lower clock: MI355X_MICROARCH.md "never compare a profiled arm with an un-profiled one")
            use_us = loop_ms * 1e3 if loop_ms else avg_us
            peak = X3_PEAK_TF if x3 else FP32_MFMA_PEAK_TF
            # `achieved` / `frac` follow the committed rocprofv3 summary (the dispatch average of the child run) whenever there is one (VERDICT r4 weak #7a);
            # the HIP-event figure of this process is carried beside it as `frac_hip_events`
            rate_us = avg_us if avg_us else use_us
            roof.update({"kernel": "den_loop_kernel (kernels/loop_fused.hpp): the whole 50-step reverse loop of the call, one launch",
                         "achieved": round(flop_loop_call / rate_us * 1e3, 2), "peak": round(peak, 1), "frac": round(flop_loop_call / rate_us * 1e3 / peak, 4),
                         "frac_hip_events": round(flop_loop_call / use_us * 1e3 / peak, 4) if loop_ms else None,
                         "achieved_hip_events": round(flop_loop_call / use_us * 1e3, 2) if loop_ms else None,
                         "peak_at_sustained_clock": round(peak * SUSTAINED_CLOCK_RATIO, 1),
                         "frac_at_sustained_clock": round(flop_loop_call / rate_us * 1e3 / (peak * SUSTAINED_CLOCK_RATIO), 4),
                         "sustained_clock_note": "peak x 1.87 / 2.4: the clock the chip holds when (nearly) every CU issues matrix instructions (measured, profiles/r05_loop_experiments.json); "
                                                 "with 160 of 256 CUs busy the loop itself runs at ~2.37 GHz, so for THIS call shape `frac` is the fairer figure and this one the floor",
                         "workgroups": (PB + 7) // 8, "cus": 256, "occupancy": round(min(1.0, (PB + 7) // 8 / 256.0), 3),
                         "frac_on_occupied_cus": round(flop_loop_call / rate_us * 1e3 / peak / min(1.0, (PB + 7) // 8 / 256.0), 4),
                         "occupancy_note": "a workgroup owns 8 motions (48 token rows = three full 16-row MFMA tiles); the kernel's run time is flat in the batch, so a call "
                                           "below 2 048 motions leaves CUs without a workgroup -- fewer motions per workgroup would not remove a row tile",
                         "gflop_per_launch": round(flop_loop_call, 1), "avg_us_rocprof_dispatch": round(avg_us, 1) if avg_us else None,
                         "avg_us_hip_events_loop_only_call": round(loop_ms * 1e3, 1) if loop_ms else None,
                         "clock": "rocprofv3 dispatch average of the child run (frac_hip_events: HIP events on the launch stream around loop-only calls of this process, which include the condition-row GEMM and the latent copies)" if avg_us else "hip_events on the launch stream, loop-only calls",
                         "frac_at_rocprof_dispatch_average": round(flop_loop_call / avg_us * 1e3 / peak, 4) if avg_us else None,
                         "dtype_of_kernel": "split-f16 x3 MFMA (roof = dense f16 MFMA peak / 3)" if x3 else "f32 MFMA",
                         "share_of_gpu_time": kern.get(loop_rows[0][0][:110], {}).get("share_of_gpu_time") if loop_rows else None})
        elif stats:
            n, (avg, calls_, total) = max(stats.items(), key=lambda kv: kv[1][2])
            roof.update({"kernel": n[:110], "achieved": None, "peak": PEAK_TF[a.precision], "frac": None, "avg_us_rocprof_dispatch": round(avg / 1e3, 2),
                         "note": "column-split kernel families (small calls): see profiles/r02_* for their per-kernel FLOP table"})
        code = kernel_code_hash(mangled_part(loop_rows[0][0])) if loop_rows else None      # the loop kernel this build launches by default
        pmc_shape, traffic_note = pmc_summary(coalesce, code)
        traffic = pmc_shape["kernels"]["den_loop"]["traffic_bytes_per_launch"] if pmc_shape and "den_loop" in pmc_shape.get("kernels", {}) else None
        roof["loop_kernel_code_hash"] = code
        roof["traffic"], roof["traffic_source"] = traffic, traffic_note
        roof["algorithmic_bytes_per_launch"] = int(STEPS_DDIM * 30.4e6 + PB * 3 * 1024 * 2)     # the weight stream once per step chip-wide + latents / condition rows
        out["roofline"] = roof
        out["kernels"] = kern
        out["decoder_roofline"] = decoder_roofline(stats, PB, pmc_shape)
        # ---- the configuration BASELINE.json names literally: one bs-64 batch at a time (latency kernels), first-class with its own roofline
        cluster = launches_single[0] <= 4
        single = {"value": round(world * BATCH / ms1["median"], 2), "unit": "motions/s", "ms_per_batch": {k: (round(v * 1e3, 4) if k != "n" else v) for k, v in ms1.items()},
                  "steps_per_repetition": K1, "launches_per_call": launches_single,
                  "shape": ("mldhip_sample, B = 64, T = 196: the reverse loop is ONE launch of 8 clusters x 24 workgroups (3 tokens x 8 column groups per 8 motions, a cluster per XCD) that "
                            "hand partial products to each other inside the launch (kernels/loop_cluster.hpp), replayed from a captured graph; decoder on the 64-row strips") if cluster else
                           "mldhip_sample, B = 64, T = 196: 2 052 dependent launches (hipGraph replay), reverse loop at 384 token rows on the latency kernels (tile32.hpp)"}
        if solo and not a.no_rocprof:
            st1, where1 = rocprof_child_stats(a.precision, 1, keep_env="MLD_BENCH_KEEP_ROCPROF_SINGLE")
            if st1:
                tot1 = sum(v[2] for v in st1.values()) or 1.0
                hits_c = [(n, v) for n, v in st1.items() if "den_cluster_kernel" in n]
                pref = "void mld::gemm_tile32_kernel<32, 1, false"          # FFN1 of the loop: norm1 on load + linear1 + GELU
                hits = [(n, v) for n, v in st1.items() if n.startswith(pref)]
                if hits_c:
                    n, (avg, calls_, total) = max(hits_c, key=lambda kv: kv[1][2])
                    gf = gf_den * STEPS_DDIM                                 # the whole loop of one bs-64 batch
                    # the kernel's own limit is not the matrix pipe: a member with a head streams ~512 KB of weight fragments per layer through its CU's L2 -> L1 path
                    # (56 B/clk/CU = 34.5 TB/s over 256 CUs, MI355X_MICROARCH.md "L2"), 3 exchanges per layer of ~2.4 us each come on top
                    wbytes = 512e3 * 9 * STEPS_DDIM
                    fill = wbytes / (avg * 1e-9) / (34.5e12 / 256)
                    cl_wgs = 8 * (24 if "8>" in n.replace(" ", "")[-12:] or ", 8>" in n else 12)      # 8 clusters x (3 tokens x column groups): the template argument of the kernel that ran
                    single["roofline"] = {"bound": "latency/l2_fill", "kernel": "den_cluster_kernel (kernels/loop_cluster.hpp): the whole 50-step reverse loop of one bs-64 batch, one launch of %d workgroups" % cl_wgs,
                                          "achieved": round(gf / (avg * 1e-9) / 1e3, 2), "peak": round(X3_PEAK_TF, 1), "peak_of": "split-f16 MFMA roof (dense f16 peak / 3)",
                                          "unit": "TFLOP/s", "frac": round(gf / (avg * 1e-9) / 1e3 / X3_PEAK_TF, 4), "avg_us_rocprof_dispatch": round(avg / 1e3, 2),
                                          "launches_per_batch": 1, "gflop_per_launch": round(gf, 2), "workgroups": cl_wgs, "cus": 256,
                                          "frac_is_against": "the split-f16 MFMA roof, for comparison with the other kernels only: the kernel is bound by hand-off latency and the per-CU L2 -> L1 fill (l2_to_cu_fill), not by the matrix pipe",
                                          "l2_to_cu_fill": {"weight_bytes_per_member_and_launch": int(wbytes), "achieved_frac_of_56_B_per_clk_per_cu": round(fill, 3),
                                                            "note": "weight stream of a member with a head (K / V for all three tokens per token member; the twelve members without a head stream 128 KB per layer) "
                                                                    "over the kernel's duration, against the per-CU L2 fill rate; the phases that stream run at ~58 B/clk, the rest of the time is hand-offs"},
                                          "share_of_gpu_time": round(total / tot1, 4), "rocprof": where1,
                                          "note": "one request cannot fill the chip: 384 token rows, 31 dependent exchanges per step; bound by hand-off latency (3 per layer, "
                                                  "~2.4 us each: profiles/r05_sync_bench.json) next to the per-CU weight stream, not by the matrix pipe (DESIGN.md, cluster loop)"}
                    ccode = kernel_code_hash(mangled_part(n))
                    pmc1, note1 = pmc_summary(1, ccode)
                    single["roofline"]["traffic"] = pmc1["kernels"]["den_cluster"]["traffic_bytes_per_launch"] if pmc1 and "den_cluster" in pmc1.get("kernels", {}) else None
                    single["roofline"]["traffic_source"], single["roofline"]["kernel_code_hash"] = note1, ccode
                    single["roofline"]["algorithmic_bytes_per_launch"] = int(STEPS_DDIM * 30.4e6 + BATCH * 3 * 1024 * 2)     # every weight once per step (the 8 XCDs' L2s each fetch their copy: x8 at most)
                elif hits:
                    n, (avg, calls_, total) = max(hits, key=lambda kv: kv[1][1])
                    gf = 2.0 * 384 * 256 * 1024 / 1e9
                    # template arguments <rows, source, transposed, PREC, ...>: PREC 1 = split-f16 MFMAs ("tile_x3"), whose roof is the f16 peak / 3
                    targs = [t.strip() for t in n.split("<", 1)[1].split(">")[0].split(",")]
                    pk1 = X3_PEAK_TF if len(targs) > 3 and targs[3] == "1" else FP32_MFMA_PEAK_TF
                    single["roofline"] = {"bound": "mfma", "kernel": "den_ffn1 = " + n[:80], "achieved": round(gf / (avg * 1e-9) / 1e3, 2), "peak": round(pk1, 1),
                                          "peak_of": "split-f16 MFMA roof (dense f16 peak / 3)" if pk1 == X3_PEAK_TF else "fp32 MFMA peak",
                                          "unit": "TFLOP/s", "frac": round(gf / (avg * 1e-9) / 1e3 / pk1, 4), "avg_us_rocprof_dispatch": round(avg / 1e3, 2),
                                          "launches_per_batch": 9 * STEPS_DDIM, "gflop_per_launch": round(gf, 4),
                                          "share_of_gpu_time": round(total / tot1, 4), "rocprof": where1,
                                          "note": "one request is a chain of 2 052 dependent launches of ~5-8 us: launch-latency bound, not MFMA bound (DESIGN.md §3 point 3 / 17c)"}
        out["single_batch"] = single
        out["bs64_pipelined"] = pipe
        out["value_single_batch"], out["ms_per_step_single_batch"] = single["value"], round(ms1["median"] * 1e3, 4)
        out["headline_shape"] = ("value_single_batch = ONE bs-64 request per call, the configuration BASELINE.json's metric is quoted on (cluster loop, kernels/loop_cluster.hpp); "
                                 "value = the serving shape, %d bs-64 requests per engine call (%d motions, %d of 256 CUs hold a workgroup of the persistent loop); "
                                 "requests_per_call_sweep carries the shapes in between" % (coalesce, PB, min(256, (PB + 7) // 8)))
        if solo:
            # ---- how the rate depends on the requests per call (the loop's run time is flat in the batch up to 2 048 motions; the decoder's is linear)
            sweep = {}
            for c_ in (1, 2, 4, 5, 10, 20, 32):
                rs = reqs_all[:c_]
                fn = (lambda: eng.sample_many(rs, stream.cuda_stream)) if c_ > 1 else (lambda: eng.sample(rs[0]["text_emb"], rs[0]["init_latents"], rs[0]["lengths"], rs[0]["latents_out"], None, rs[0]["joints_out"], stream.cuda_stream))
                fn(); fn()
                torch.cuda.synchronize()
                ts = []
                for _ in range(3):
                    t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
                sweep[str(c_)] = {"motions_per_call": BATCH * c_, "ms_per_call": round(min(ts) * 1e3, 3), "value": round(BATCH * c_ / min(ts), 1),
                                  "loop_workgroups": (BATCH * c_ + 7) // 8 if BATCH * c_ > 256 else None}
            out["requests_per_call_sweep"] = {"unit": "motions/s", "note": "one call at a time, best of 3; loop_workgroups = workgroups of the persistent loop "
                                              "(None: calls of up to 256 motions run the cluster loop -- one launch up to 128 motions, two above)", "shapes": sweep}
            # ---- BASELINE config 3 (512 prompts over 8 ranks) as seen by ONE rank: its share is one bs-64 batch (world 8) or all 512 (world 1)
            rs512 = reqs_all[:8]
            eng.sample_many(rs512, stream.cuda_stream)
            t512 = min(run_steps(lambda i, st: eng.sample_many(rs512, stream.cuda_stream), 1, [None]) for _ in range(3))
            out["config3_per_rank"] = {"unit": "motions/s per rank", "world_1_512_prompts_one_call": round(512 / t512, 1),
                                       "world_8_64_prompts_per_rank": single["value"],
                                       "world_8_aggregate_if_linear": round(8 * single["value"], 1),
                                       "note": "DataParallelSampler picks the requests per call by itself (shard size vs engine max_batch); on 8 ranks each rank's share of config 3 "
                                               "is ONE bs-64 batch, i.e. the single_batch path: 8 x that is the config-3 rate to expect on an 8-GPU node (no data-path collective)"}

        cj = None
        if world == 1 and not a.no_cpu_baseline:
            # MKL/OpenMP oversubscribes badly on a 256-thread host with these small GEMMs: three thread counts, the best one is the baseline
            # (VERDICT r3 weak #6c: 32 threads alone understated it); ~5 s of CPU work each
            ncpu = os.cpu_count() or 1
            tries = {}
            info, cj = None, None
            for th in sorted({min(16, ncpu), min(32, ncpu), min(64, ncpu)}):
                inf_, cj_ = cpu_baseline(1234 + rank, th)
                if cj_ is None:
                    continue
                tries[str(th)] = round(inf_["motions_per_s"], 2)
                if info is None or inf_["motions_per_s"] > info["motions_per_s"]:
                    info, cj = inf_, cj_
            threads = info["threads"] if info else min(32, ncpu)
            if cj is not None:
                out["cpu_baseline"] = {"value": round(info["motions_per_s"], 2), "unit": "motions/s", "cores": info["threads"],
                                       "kind": "port", "host_cpus": info["cores"], "motions_per_s_by_threads": tries,
                                       "sample": "1 batch of 64 motions (T=196, 50 steps) through oracle.mld_oracle (torch-CPU backend), %.1f s, best of the thread counts tried" % info["seconds"],
                                       "reference_modules_survey": {
                                           "value": 15.2, "unit": "motions/s", "cores": 8, "host": "survey sandbox, Xeon 2.1 GHz, MKL",
                                           "provenance": "SURVEY.md §8(d) probe: the reference's own MldDenoiser / MldVae modules + restated DDIM at B=64 "
                                                         "(4.2 s per batch); /root/reference cannot travel to the GPU box, so it is not re-timed here"}}
            else:
                out["cpu_baseline"] = {"value": None, "unit": "motions/s", "cores": threads, "kind": "port", "sample": "the oracle child failed or timed out"}
            # the same array code on stock ATen kernels of the SAME GPU (SURVEY.md §7.2b "PyTorch-ROCm eager motions/s on the same GPU")
            info_g, jg = cpu_baseline(1234 + rank, threads, device="cuda", repeat=3)
            if jg is not None:
                out["eager_same_gpu"] = {"value": round(info_g["motions_per_s"], 2), "unit": "motions/s", "kind": "oracle.mld_oracle.TorchOps on cuda: plain PyTorch-ROCm eager, fp32, "
                                         "one bs-64 batch (T=196, 50 steps), best of 3; NOT the reference's nn.Modules (they cannot travel), the same arithmetic graph",
                                         "seconds_per_batch": round(info_g["seconds"], 4),
                                         "max_abs_joints_vs_cpu_oracle": float(np.abs(jg - cj).max()) if cj is not None else None}
            else:
                out["eager_same_gpu"] = {"value": None, "error": str(info_g)}
        if solo:
            # ---- parity of the headline call, ALL of it: every request against the exact-fp32 engine on the latency kernels (itself
            #      within ~1e-4 of the reference fixture, tests/test_gpu_parity.py), request 0 against the CPU oracle run above
            issue(eng)
            torch.cuda.synchronize()
            got = [r["joints_out"].clone() for r in reqs]
            ex = make_engine(local, weights, "f32", max_batch=BATCH)
            worst, per = 0.0, []
            jbuf = torch.empty(BATCH, FRAMES, 22, 3, device=dev)
            for r, g_ in zip(reqs, got):
                ex.sample(r["text_emb"], r["init_latents"], r["lengths"], None, None, jbuf, stream.cuda_stream)
                torch.cuda.synchronize()
                per.append(round(float((g_ - jbuf).abs().max()), 7))
            worst = max(per)
            issue_single(eng, 1)                 # request 0 again, alone, on the latency kernels of the headline mode
            ex.sample(reqs[0]["text_emb"], reqs[0]["init_latents"], reqs[0]["lengths"], None, None, jbuf, stream.cuda_stream)
            torch.cuda.synchronize()
            j_single, j_exact = reqs[0]["joints_out"].cpu().numpy(), jbuf.cpu().numpy()
            par = {"tolerance": 1e-3, "precision": a.precision, "motions_checked": PB,
                   "max_abs_joints_vs_exact_fp32_engine_all_requests": worst, "per_request": per,
                   "max_abs_joints_vs_exact_fp32_engine_single_call": float(np.abs(j_single - j_exact).max())}
            if cj is not None:
                par["max_abs_joints_vs_oracle_request0_of_headline_call"] = float(np.abs(got[0].cpu().numpy() - cj).max())
                par["max_abs_joints_vs_oracle_single_call"] = float(np.abs(j_single - cj).max())
                par["max_abs_joints_vs_oracle"] = max(par["max_abs_joints_vs_oracle_request0_of_headline_call"], par["max_abs_joints_vs_oracle_single_call"])
                par["exact_fp32_engine_vs_oracle_request0"] = float(np.abs(j_exact - cj).max())
            out["parity"] = par
            ex.close()
        if solo and not a.no_alt:
            # ---- the other arithmetic modes on the same workload and timing rule, each with its measured error
            alts = {}
            for prec in [p for p in ("f32", "f16x3", "bf16") if p != a.precision]:
                e2 = make_engine(local, weights, prec, max_batch=PB)
                issue(e2)
                fused2 = e2.launch_counts()[0] <= 4
                issue_single(e2, 2)
                torch.cuda.synchronize()
                t4 = min(run_steps(lambda i, st: issue(e2), 1, [None]) for _ in range(3))
                t1 = run_steps(lambda i, st: issue_single(e2, 1), 8, [None]) / 8
                alt = {"value": round(BATCH * K / t4, 2), "value_single_batch": round(BATCH / t1, 2), "dtype": DTYPE[prec],
                       "loop": "sample-major persistent launch" if fused2 else "column-split throughput kernels (strip.hpp): the persistent loop is built for fp32 / split-f16 operands"}
                if fused2:
                    e2.sample_many(lat_only, stream.cuda_stream)
                    lm_ = min(events_ms(stream, lambda: e2.sample_many(lat_only, stream.cuda_stream))[0] for _ in range(3))
                    pk = FP32_MFMA_PEAK_TF if prec == "f32" else X3_PEAK_TF
                    alt["loop_kernel_roofline"] = {"avg_us_hip_events_loop_only_call": round(lm_ * 1e3, 1), "achieved_tflops": round(flop_loop_call / lm_, 2),
                                                   "peak": round(pk, 1), "frac": round(flop_loop_call / lm_ / pk, 4)}
                if cj is not None:
                    issue(e2)
                    torch.cuda.synchronize()
                    alt["max_abs_joints_vs_oracle"] = float(np.abs(reqs[0]["joints_out"].cpu().numpy() - cj).max())
                alts[prec] = alt
                e2.close()
            out["alt_modes"] = alts
            # ---- round 2's serving shape for continuity: 5 requests per call on the column-split throughput kernels, 4 calls in flight
            nfl, c2 = 4, 5
            e5 = make_engine(local, weights, a.precision, max_batch=BATCH * c2, nfl=nfl)
            e5.set_option("loop_kernel", 2)
            streams = [torch.cuda.Stream(device=dev) for _ in range(nfl)]
            r5 = make_requests(dev, c2 * nfl, 7)
            call5 = lambda i, st: e5.sample_many(r5[(i % nfl) * c2:(i % nfl) * c2 + c2], streams[i % nfl].cuda_stream)
            run_steps(call5, 2 * nfl, [None])
            t5 = run_steps(call5, 8, [None])
            out["round2_shape"] = {"value": round(BATCH * c2 * 8 / t5, 2), "unit": "motions/s", "requests_per_call": c2, "calls_in_flight": nfl,
                                   "note": "5 x 64 motions per call on the column-split throughput kernels (strip.hpp), 4 calls in flight on 4 streams: round 2's headline shape, this round's build"}
            e5.close()
        if solo:
            # also a realistic length mix -- uniform in {40, 44, ..., 196}, seed 1234 (same Tmax, ragged masks)
            rng = np.random.Generator(np.random.PCG64(1234))
            mix = [[int(v) for v in rng.choice(np.arange(40, 197, 4), BATCH)] for _ in range(len(reqs))]
            for ln in mix:
                ln[0] = FRAMES                                  # keep Tmax = 196 so buffers / graphs are the same
            issue(eng, mix)
            dtm = min(run_steps(lambda i, st: issue(eng, mix), 1, [None]) for _ in range(3))
            lm = {"value": round(BATCH * K / dtm, 2), "unit": "motions/s", "ms_per_step": round(dtm / K * 1e3, 4),
                  "lengths": "uniform in {40..196 step 4}, seed 1234, Tmax 196; mean %.1f frames" % float(np.mean(mix))}
            if not a.no_cpu_baseline:
                lf = "/tmp/mld_bench_lengths_%d.json" % os.getpid()
                json.dump(mix[0], open(lf, "w"))
                info, jm = cpu_baseline(1234 + rank, min(32, os.cpu_count() or 1), lengths_file=lf)
                if jm is not None:
                    issue(eng, mix)
                    torch.cuda.synchronize()
                    j = reqs[0]["joints_out"].cpu().numpy()
                    lm["max_abs_joints_vs_oracle"] = float(max(np.abs(j[i, :n] - jm[i, :n]).max() for i, n in enumerate(mix[0])))
                    lm["tolerance"] = 1e-3
            out["length_mix"] = lm
        if solo:
            out["other_workloads"] = []
            s2 = [torch.cuda.Stream(device=dev) for _ in range(2)]
            if not a.no_a2m:
                out["other_workloads"].append(bench_a2m(local, dev, 2, 8, s2))
            if not a.no_novae:
                out["other_workloads"].append(bench_novae(local, dev, a.novae_full_length, s2))
        if world == 1 and not a.no_clip:
            try:
                te = bench_text_encoder(dev)
                te["single_batch_motions_per_s_incl_text"] = round(BATCH / (out["ms_per_step_single_batch"] + te["ms_per_128_prompts"]) * 1e3, 1)
                te["note"] = "text encoding of a batch can overlap the sampling of the batches already queued; this is the strictly serial view"
                out["text_encoder"] = te
            except Exception as ex_:  # transformers missing / API drift: report, never fail the bench
                out["text_encoder"] = {"error": repr(ex_)[:200]}
    if rank == 0:
        emit(out)
    if dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
