"""Shared pieces of the batch-size edge tests (tests/test_gpu_batch_edges.py on the MI355X, tests/test_batch_edges_sim.py on the simulator): the number of
motions B of a call decides which reverse-loop kernels run, on which tile height, in how many launches -- the lists below sit on those edges.

Reference.  One batch of `bmax` motions per (weights, steps) is run once on the three backends of tests/config_envelope_ref.py (float64, and the two float32
evaluations whose larger error is e32); the motions of a call are independent, so a call of B motions is the first B unconditional rows followed by the
first B conditional rows of that batch (call_inputs) and its reference the first B rows of the result (prefix).  Tolerances are the project's own: the
relative rule of config_envelope_ref.Record.rule for eta = 0 latents, ETA_TOL (tests/test_gpu_ddim_eta.py's latent bound) for stochastic calls against the
float32 numpy loop fed the same Philox draws."""
import numpy as np

import config_envelope_ref as R
from mld_hip import synthetic as syn
from oracle import mld_oracle as O

GUIDANCE = 7.5
MAX_FRAMES, LENGTH = 16, 8          # latents only: the decoder is not part of these tests
ETA_TOL = 5e-3                      # tests/test_gpu_ddim_eta.py: final latents of a stochastic call against the float32 numpy loop

# latency kernels (kernels/tile32.hpp tile32(), M = 6B token rows): 16-row tiles while ceil(6B / 16) x ceil(N / 64) x nz <= 256.  N = 256: FFN2 (nz 4) switches
# to 32-row tiles at B = 42 | 43, the skip linear (nz 2) at 85 | 86, the out-projection with its in-register 3-token attention (nz 1) at 170 | 171; the wider
# GEMMs (in-projection, FFN1) always run 32-row tiles, whose last tile has an empty second half at B = 3 and 8 (18 and 48 rows); B = 1, 2 are one partial 16-row tile.  191 after 1: the largest call
# auto gives these kernels on an F16X3 handle, on workspace rows the small calls wrote.
LATENCY_BS = [171, 170, 86, 85, 43, 42, 8, 6, 5, 3, 2, 1, 191]
# column-split throughput kernels (kernels/strip.hpp strip(), 32-row tiles): auto runs them on an F32 handle from 128 ("strip_min_rows" 768 = 6 x 128) to
# 1 279 motions (the persistent loop from 1 280)
THROUGHPUT_BS = [1279, 171, 129, 128, 127, 16, 11, 6, 5, 1]
# persistent loop (kernels/loop_fused.hpp): one workgroup per 8 motions, grid = ceil(B / 8); above 8 x 256 CUs = 2 048 motions workgroups take a second round
PERSISTENT_BS = [2049, 2048, 2041, 17, 16, 9, 8, 7, 1]
# cluster loop (kernels/loop_cluster.hpp): 8 column groups up to 64 motions (8 clusters) and 4 above, launches of up to 128 motions, grid = 8 x members x
# ceil(clusters / 8): 57 .. 65 the last full / first idle cluster slots and the switch of the form, 72 | 73 the 9 | 10 clusters of the 4-group form, 129 a second
# launch of one motion, 255 | 256 the ragged and the full second launch
CLUSTER_BS = [256, 255, 129, 128, 127, 73, 72, 65, 64, 57, 9, 8, 1]
CLUSTER_G4_BS = [64, 9, 1]

KEY_SEED = 0xFEDCBA9876543210
# first_index of the noise keys (include/mldhip.h "Noise contract": quad = index * 64 + q).  With 11 motions the first three put quad 2^31, quad 2^32 and
# index 2^31 inside the call; the last has a quad above 2^46
KEY_INDICES = [2 ** 25 - 4, 2 ** 26 - 4, 2 ** 31 - 4, 2 ** 40 + 3]
KEY_MOTIONS = 11

_ref = {}


def steps_for(B):
    """4 steps up to 257 motions, 2 above (both divide 1000; more than one, so that the state carried between steps is exercised)"""
    return 4 if B <= 257 else 2


def batch(bmax, seed=131):
    key = ("batch", bmax, seed)
    if key not in _ref:
        _ref[key] = syn.make_batch(bmax, [LENGTH] * bmax, seed=seed)
    return _ref[key]


def loop_reference(weights, steps, bmax, tag="default"):
    """the final latents [bmax, 1, 256] of the reverse loop on the batch of bmax motions: [fp64, NumpyOps(float32), TorchOps('float32')], computed once"""
    key = ("loop", tag, steps, bmax)
    if key not in _ref:
        b = batch(bmax)
        outs = []
        for ops in R.backends():
            lat = O.diffusion_reverse(ops, O.to_backend(ops, weights[0]), ops.asarray(b.text_emb), ops.asarray(b.init_latents), GUIDANCE, steps, 4)
            outs.append(np.asarray(lat if isinstance(lat, np.ndarray) else ops.to_numpy(lat), np.float64))
        for o in outs:
            o.setflags(write=False)
        _ref[key] = outs
    return _ref[key]


def call_inputs(bmax, B):
    """(text_emb [2B, 1, 768], init_latents [B, 1, 256], lengths) of the call of the first B motions of the batch of bmax"""
    b = batch(bmax)
    text = np.ascontiguousarray(np.concatenate([b.text_emb[:B], b.text_emb[bmax:bmax + B]], 0))
    return text, np.ascontiguousarray(b.init_latents[:B]), [LENGTH] * B


def prefix(outs, B):
    """(fp64 latents, e32) of the first B motions"""
    r64 = outs[0][:B]
    return r64, max(float(np.abs(o[:B] - r64).max()) for o in outs[1:])


def philox_quad_scalar(seed, step, quad):
    """Philox4x32-10 + Box-Muller of one quad on Python integers (no array arithmetic): the independent check of oracle.philox_normal's `first` at counters
    above 2^32, where no prefix stream can be generated"""
    c = [quad & 0xFFFFFFFF, (quad >> 32) & 0xFFFFFFFF, step, 0]
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = O.PHILOX_M0 * c[0], O.PHILOX_M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k1, p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + O.PHILOX_W0) & 0xFFFFFFFF, (k1 + O.PHILOX_W1) & 0xFFFFFFFF
    u = [((x >> 8) + 0.5) / 16777216.0 for x in c]
    r0, r1 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    t0, t1 = 2 * np.pi * u[1], 2 * np.pi * u[3]
    return np.array([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1), r1 * np.sin(t1)])


def key_batch():
    """the 11 motions of the noise-key cases"""
    return syn.make_batch(KEY_MOTIONS, [LENGTH] * KEY_MOTIONS, seed=132)


def cluster_launches(B):
    """condition rows + one cluster launch per 128 motions"""
    return 1 + (B + 127) // 128
