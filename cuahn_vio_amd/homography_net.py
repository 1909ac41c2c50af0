"""Host-side mirror of the reference runtime class ``pytorch::HomographyNet``
(reference cuahn_ros/homography_network/src/HomographyNet.h:23-67, HomographyNet.cpp) and a batched engine,
both thin wrappers over the C ABI of include/hnet.h (libhnet_hip.so).  No torch on this path.

``HomographyNet`` keeps the reference's method names, argument meaning and "print and carry on" error
behaviour so the parity tests read like a port of the reference's call sites
(cuahn/src/core/VioManager.cpp:188,236,258-259).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _capi
from ._capi import PIX_F32, PIX_U8, Config, HnetError, Timing, check, lib  # noqa: F401

HIP_STREAM_LEGACY = 1      # hipStreamLegacy ((hipStream_t)1, hip_runtime_api.h): the NULL / default stream, named explicitly

IMG_H, IMG_W = 224, 320
VARIANTS = {"full": (0, 3), "prior3": (1, 3), "prior2": (1, 2), "prior1": (1, 1)}


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


IGNORE_ENV = False      # bench.py sets this (unless --honour-env): engines are then built from explicit arguments only, a stray HNET_* variable cannot change the timed kernels


def env_overrides():
    """the HNET_* variables of this process that kernel_selection_from_env / HnetEngine would map onto hnet_config (what bench.py lists in `env_overrides`)"""
    names = ("HNET_S3_TILE", "HNET_FUSE_SMALL", "HNET_FUSE_B3", "HNET_FUSE_B42", "HNET_CHAIN", "HNET_CHAIN_GRID", "HNET_CHAIN_FC", "HNET_WARP_FUSE", "HNET_GRAPH_COPIES", "HNET_GRAPH", "HNET_WARP_EXACT", "HNET_PRECISION")
    return {n: os.environ[n] for n in names if n in os.environ}


def kernel_selection_from_env():
    """hnet_config.warp_exact / .graph / .variant from this process's environment.  The C library reads no environment variable (round 4);
    the test suite and tools/ab_bench.py keep selecting reference kernels with HNET_WARP_EXACT, HNET_GRAPH (0 eager, 1 replay also in the timing
    entry point), HNET_S3_TILE (13 / 20 / 21 / 22 / 25 / 30: include/hnet.h HNET_VARIANT_*), HNET_FUSE_SMALL=0, HNET_FUSE_B3=0, HNET_FUSE_B42=0 - mapped here."""
    if IGNORE_ENV:
        return 0, 0, 0
    env = os.environ.get
    variant = int(env("HNET_S3_TILE", "0")) & 0xff
    if env("HNET_FUSE_SMALL", "1") == "0":
        variant |= 1 << 8
    if env("HNET_FUSE_B3", "1") == "0":
        variant |= 1 << 9
    if env("HNET_FUSE_B42", "1") == "0":
        variant |= 1 << 10
    if env("HNET_CHAIN", "1") == "0":       # the per-layer launches instead of the one-XCD tail chains of the latency path (include/hnet.h HNET_VARIANT_NO_CHAIN)
        variant |= 1 << 11
    if env("HNET_CHAIN_GRID", "") in ("8", "3"):      # tests: the chain launches with 8 / 3 workgroups (HNET_VARIANT_CHAIN_GRID_*)
        variant |= (1 << 12) if env("HNET_CHAIN_GRID") == "8" else (1 << 13)
    if env("HNET_CHAIN_FC", "1") == "0":    # the block-tail FC recomputed by the next warp + pool launch instead of summed from the chain's partial sums (HNET_VARIANT_CHAIN_NO_FC)
        variant |= 1 << 16
    if env("HNET_WARP_FUSE", "0") == "1":   # opt-in: block 4's warp + concat sampled inside the block_4_0 + block_4_1 kernel (include/hnet.h HNET_VARIANT_WARP_FUSE)
        variant |= 1 << 14
    if env("HNET_GRAPH_COPIES", "0") == "1":   # hnet_infer's graph with memcpy nodes instead of kernels that read / write the pinned host block (HNET_VARIANT_GRAPH_COPIES)
        variant |= 1 << 15
    graph = {"0": 1, "1": 2}.get(env("HNET_GRAPH", ""), 0)
    return int(env("HNET_WARP_EXACT", "0") != "0"), graph, variant


FROM_FILE = -1      # include/hnet.h HNET_FROM_FILE


def make_config(variant="full", mc_samples=16, dropout_p=0.05, mc_seed=0, max_batch=1, emit_error_map=False, device_id=0, mc_shard=None, precision=None):
    """hnet_config from the arguments of HnetEngine / HnetGroup (None = HNET_FROM_FILE where the C ABI has it) and this process's kernel-selection environment"""
    cfg = Config()
    lib().hnet_default_config(C.byref(cfg))
    if precision is None:   # default: the library's (fp16 planes, fp32-grade); HNET_PRECISION=2 / 0 select split-bf16 / the exact-fp32 MFMA path
        precision = cfg.precision if IGNORE_ENV else int(os.environ.get("HNET_PRECISION", str(cfg.precision)))
    cfg.device_id = device_id
    cfg.use_prior, cfg.blocks_to_run = VARIANTS[variant] if variant is not None else (FROM_FILE, FROM_FILE)
    cfg.mc_samples = FROM_FILE if mc_samples is None else mc_samples
    cfg.dropout_p = -1.0 if dropout_p is None else dropout_p
    cfg.mc_seed = mc_seed
    cfg.emit_error_map, cfg.precision, cfg.max_batch = (FROM_FILE if emit_error_map is None else int(emit_error_map)), precision, max_batch
    if mc_shard is not None:
        cfg.mc_sample_begin, cfg.mc_sample_end = mc_shard
    cfg.warp_exact, cfg.graph, cfg.variant = kernel_selection_from_env()
    return cfg


class HnetEngine:
    """One hnet context (one GPU).  `weights` is an HNETW001 blob (bytes) or a path to one."""

    def __init__(self, weights, variant="full", mc_samples=16, dropout_p=0.05, mc_seed=0, max_batch=1,
                 emit_error_map=False, device_id=0, mc_shard=None, precision=None):
        """variant / mc_samples / dropout_p / emit_error_map = None: HNET_FROM_FILE - taken from the blob's `hnet.variant` record
        (cuahn_vio_amd.weights.pack_state_dict(..., variant=...)); `config()` returns what is in effect"""
        L = lib()
        cfg = make_config(variant, mc_samples, dropout_p, mc_seed, max_batch, emit_error_map, device_id, mc_shard, precision)
        self.cfg, self.variant, self._L = cfg, variant, L
        self._owned = True
        self._h = C.c_void_p()
        if isinstance(weights, (bytes, bytearray)):
            buf = (C.c_char * len(weights)).from_buffer_copy(weights)
            rc = L.hnet_create_from_memory(C.byref(cfg), C.cast(buf, C.c_void_p), len(weights), C.byref(self._h))
        else:
            rc = L.hnet_create(C.byref(cfg), str(weights).encode(), C.byref(self._h))
        check(None, rc)
        used = self.config()
        if variant is None:
            self.variant = {(0, 3): "full", (1, 3): "prior3", (1, 2): "prior2", (1, 1): "prior1"}[(used.use_prior, used.blocks_to_run if used.use_prior else 3)]
        self.n_local = (cfg.mc_sample_end - cfg.mc_sample_begin) if mc_shard else used.mc_samples

    def config(self):
        """hnet_get_config: the configuration in effect (HNET_FROM_FILE fields resolved from the blob)"""
        out = Config()
        check(self._h, self._L.hnet_get_config(self._h, C.byref(out)))
        return out

    def precision(self):
        """the arithmetic mode in effect (hnet_precision: HNET_PREC_F16X2 falls back to HNET_PREC_BF16X3 outside the fp16 range)"""
        return int(self._L.hnet_precision(self._h))

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self, "_owned", True):
                self._L.hnet_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    @classmethod
    def _borrow(cls, handle, variant=None):
        """a view of a context somebody else owns (a member of an HnetGroup): every method works, close() does not destroy"""
        e = cls.__new__(cls)
        e._L, e._h, e._owned, e.variant = lib(), C.c_void_p(handle), False, variant
        e.cfg = e.config()
        e.n_local = (e.cfg.mc_sample_end - e.cfg.mc_sample_begin) or e.cfg.mc_samples
        return e

    @property
    def handle(self):
        return self._h

    # ---- batched inference, host buffers -------------------------------------------------------
    def infer_batch(self, prev, curr, prior=None, pair_seq0=0, want_err=False):
        prev, curr = np.ascontiguousarray(prev), np.ascontiguousarray(curr)
        if prev.dtype != curr.dtype or prev.dtype not in (np.uint8, np.float32):
            raise TypeError("images must both be uint8 or float32")
        fmt = PIX_U8 if prev.dtype == np.uint8 else PIX_F32
        b = prev.reshape(-1, IMG_H, IMG_W).shape[0]
        mean = np.zeros((b, 8), np.float32)
        cov = np.zeros((b, 8, 8), np.float32)
        err = np.zeros((b, IMG_H, IMG_W), np.float32) if want_err else None
        pr = None if prior is None else np.ascontiguousarray(prior, dtype=np.float32).reshape(b, 8)
        rc = self._L.hnet_infer_batch(self._h, prev.ctypes.data, curr.ctypes.data, fmt, _fp(pr) if pr is not None else None,
                                      b, pair_seq0, _fp(mean), _fp(cov), _fp(err) if want_err else None)
        check(self._h, rc)
        return (mean, cov, err) if want_err else (mean, cov)

    # ---- device-resident entry points (raw device pointers, e.g. torch tensors' data_ptr()) ------
    @staticmethod
    def _stream(stream):
        """stream argument of the device entry points: None -> the context's own stream (C ABI: NULL); a torch.cuda.Stream
        or a raw hipStream_t handle -> that stream.  The handle 0 is torch's name for the legacy default stream; the C ABI
        reserves NULL for "context stream", so 0 is passed as hipStreamLegacy ((hipStream_t)1) — the kernels then run in
        order with torch's default-stream work (tensor fills, RCCL collectives)."""
        if stream is None:
            return None
        h = getattr(stream, "cuda_stream", stream)
        return HIP_STREAM_LEGACY if int(h) == 0 else int(h)

    def infer_batch_device(self, d_prev, d_curr, fmt, d_prior, batch, pair_seq0, d_mean, d_cov, d_err=None, stream=None):
        check(self._h, self._L.hnet_infer_batch_device(self._h, d_prev, d_curr, fmt, d_prior, batch, pair_seq0, d_mean, d_cov,
                                                       d_err, self._stream(stream)))

    def infer_batch_packed_device(self, d_prev, d_curr, fmt, d_prior, batch, pair_seq0, d_out72, d_err=None, stream=None):
        """the same forward with the packed [batch, 72] record (mean | cov) as output: the message of the multi-GPU gather, written by the ensemble kernel"""
        check(self._h, self._L.hnet_infer_batch_packed_device(self._h, d_prev, d_curr, fmt, d_prior, batch, pair_seq0, d_out72, d_err, self._stream(stream)))

    def infer_batch_seqs_packed_device(self, d_prev, d_curr, fmt, d_prior, batch, d_pair_seq, d_out72, d_err=None, stream=None):
        """infer_batch_packed_device with one mask sequence number per pair: d_pair_seq = device uint64 [batch] (pair b's key; [s0, s0 + 1, ...] = pair_seq0 s0)"""
        check(self._h, self._L.hnet_infer_batch_seqs_packed_device(self._h, d_prev, d_curr, fmt, d_prior, batch, d_pair_seq, d_out72, d_err,
                                                                   self._stream(stream)))

    def mc_finish_packed_device(self, d_mean_s, d_logvar_s, n_total, d_h1, batch, d_out72, stream=None):
        check(self._h, self._L.hnet_mc_finish_packed_device(self._h, d_mean_s, d_logvar_s, n_total, d_h1, batch, d_out72, self._stream(stream)))

    def infer_mc_partial_device(self, d_prev, d_curr, fmt, d_prior, batch, pair_seq0, d_mean_s, d_logvar_s, d_h1, stream=None):
        check(self._h, self._L.hnet_infer_mc_partial_device(self._h, d_prev, d_curr, fmt, d_prior, batch, pair_seq0, d_mean_s,
                                                            d_logvar_s, d_h1, self._stream(stream)))

    def mc_finish_gathered_device(self, d_gathered, world, n_local, d_h1, batch, d_out72, stream=None):
        """hnet_mc_finish_gathered_device: the ensemble straight from the all-gathered [world][2][B][n_local][8] buffer"""
        check(self._h, self._L.hnet_mc_finish_gathered_device(self._h, d_gathered, world, n_local, d_h1, batch, d_out72, self._stream(stream)))

    def mc_finish_device(self, d_mean_s, d_logvar_s, n_total, d_h1, batch, d_mean, d_cov, stream=None):
        check(self._h, self._L.hnet_mc_finish_device(self._h, d_mean_s, d_logvar_s, n_total, d_h1, batch, d_mean, d_cov,
                                                     self._stream(stream)))

    def synchronize(self, stream=None):
        check(self._h, self._L.hnet_synchronize(self._h, self._stream(stream)))

    def overflow_flag(self, stream=None):
        """hnet_overflow_flag: synchronises, returns and clears the device word the forwards OR into when an output is not finite (bit 0).
        The device-resident entry points cannot look at their results; in HNET_PREC_F16X2 a set bit with finite inputs means an
        activation left the fp16-plane range and the batch should be repeated on a HNET_PREC_BF16X3 context."""
        v = C.c_int(0)
        check(self._h, self._L.hnet_overflow_flag(self._h, self._stream(stream), C.byref(v)))
        return int(v.value)

    def time_batch_device(self, d_prev, d_curr, fmt, d_prior, batch, pair_seq0, d_mean, d_cov, iters):
        per = np.zeros(iters, np.float32)
        tot = C.c_float(0)
        check(self._h, self._L.hnet_time_batch_device(self._h, d_prev, d_curr, fmt, d_prior, batch, pair_seq0, d_mean, d_cov,
                                                      iters, _fp(per), C.byref(tot)))
        return per, float(tot.value)

    def stages(self):
        n = self._L.hnet_stage_count(self._h)
        return [(self._L.hnet_stage_name(self._h, i).decode(), self._L.hnet_stage_flops_per_pair(self._h, i)) for i in range(n)]

    def stage_kernels(self):
        """kernels per stage of the last profiled forward (hnet_stage_kernels: a split-K layer with a separate reduce launch counts 2)"""
        return [int(self._L.hnet_stage_kernels(self._h, i)) for i in range(self._L.hnet_stage_count(self._h))]

    def profile_batch_device(self, d_prev, d_curr, fmt, d_prior, batch, pair_seq0, d_mean, d_cov, iters):
        ms = np.zeros(self._L.hnet_stage_count(self._h), np.float32)
        check(self._h, self._L.hnet_profile_batch_device(self._h, d_prev, d_curr, fmt, d_prior, batch, pair_seq0, d_mean, d_cov,
                                                         iters, _fp(ms)))
        return ms

    def last_timing(self):
        t = Timing()
        check(self._h, self._L.hnet_last_timing(self._h, C.byref(t)))
        return {"device_ms": t.device_ms, "host_ms": t.host_ms, "n_inferences": t.n_inferences,
                "sum_device_ms_after_100": t.sum_device_ms_after_100, "n_main_inferences": t.n_main_inferences}

    # ---- operator-level entry points (NCHW host arrays, like the reference tensors) ---------------
    def op_warp(self, img, h):
        img = np.ascontiguousarray(img, dtype=np.float32).reshape(IMG_H, IMG_W)
        hm = np.ascontiguousarray(h, dtype=np.float32).reshape(9)
        out = np.zeros((IMG_H, IMG_W), np.float32)
        check(self._h, self._L.hnet_op_warp(self._h, _fp(img), _fp(hm), _fp(out)))
        return out

    def op_dlt(self, dst):
        d = np.ascontiguousarray(dst, dtype=np.float32).reshape(-1, 8)
        out = np.zeros((d.shape[0], 3, 3), np.float32)
        check(self._h, self._L.hnet_op_dlt(self._h, _fp(d), d.shape[0], _fp(out)))
        return out

    def op_photo_residual(self, img1, img2, offsets, want_map=False):
        """photometric residual records (hnet_op_photo_residual): img1 / img2 uint8 [n, 224, 320], offsets [n, m, 8] pixels ->
        records [n, m] of _capi.PHOTO_RESIDUAL_DTYPE (, the error map itself [n, m, 224, 320] float32)"""
        a = np.ascontiguousarray(img1, dtype=np.uint8).reshape(-1, IMG_H, IMG_W)
        b = np.ascontiguousarray(img2, dtype=np.uint8).reshape(-1, IMG_H, IMG_W)
        n = a.shape[0]
        if b.shape[0] != n:
            raise ValueError("img1 and img2 must hold the same number of frames")
        off = np.ascontiguousarray(offsets, dtype=np.float32).reshape(n, -1, 8)
        m = off.shape[1]
        out = np.zeros((n, m), _capi.PHOTO_RESIDUAL_DTYPE)
        emap = np.zeros((n, m, IMG_H, IMG_W), np.float32) if want_map else None
        check(self._h, self._L.hnet_op_photo_residual(self._h, a.ctypes.data, b.ctypes.data, n, _fp(off), m, out.ctypes.data,
                                                      emap.ctypes.data if want_map else None))
        return (out, emap) if want_map else out

    def op_photo_align(self, img1, img2, offsets0, **opts):
        """photometric alignment (hnet_op_photo_align): img1 / img2 uint8 [n, 224, 320], start offsets [n, 8] pixels; opts: the fields of
        hnet_photo_align_opts (max_iterations, min_valid, lambda0, eps_px) -> records [n] of _capi.PHOTO_ALIGN_DTYPE"""
        a = np.ascontiguousarray(img1, dtype=np.uint8).reshape(-1, IMG_H, IMG_W)
        b = np.ascontiguousarray(img2, dtype=np.uint8).reshape(-1, IMG_H, IMG_W)
        n = a.shape[0]
        if b.shape[0] != n:
            raise ValueError("img1 and img2 must hold the same number of frames")
        off = np.ascontiguousarray(offsets0, dtype=np.float32).reshape(n, 8)
        o = _capi.photo_align_opts(**opts)
        out = np.zeros(n, _capi.PHOTO_ALIGN_DTYPE)
        check(self._h, self._L.hnet_op_photo_align(self._h, a.ctypes.data, b.ctypes.data, n, off.ctypes.data, C.addressof(o), out.ctypes.data))
        return out

    def op_photo_align_pyramid(self, img1, img2, offsets0, levels=4, want_levels=False, **opts):
        """coarse-to-fine photometric alignment (hnet_op_photo_align_pyramid): as op_photo_align, one complete alignment per pyramid level from
        levels - 1 down to 0 (max_iterations is per level) -> the level-0 records [n]; want_levels: (those, every level's records [n, levels],
        index = level)"""
        a = np.ascontiguousarray(img1, dtype=np.uint8).reshape(-1, IMG_H, IMG_W)
        b = np.ascontiguousarray(img2, dtype=np.uint8).reshape(-1, IMG_H, IMG_W)
        n = a.shape[0]
        if b.shape[0] != n:
            raise ValueError("img1 and img2 must hold the same number of frames")
        off = np.ascontiguousarray(offsets0, dtype=np.float32).reshape(n, 8)
        o = _capi.photo_align_opts(**opts)
        out = np.zeros(n, _capi.PHOTO_ALIGN_DTYPE)
        lv = np.zeros((n, max(int(levels), 1)), _capi.PHOTO_ALIGN_DTYPE) if want_levels else None
        check(self._h, self._L.hnet_op_photo_align_pyramid(self._h, a.ctypes.data, b.ctypes.data, n, off.ctypes.data, C.addressof(o), int(levels),
                                                           out.ctypes.data, lv.ctypes.data if want_levels else None))
        return (out, lv) if want_levels else out

    def op_photo_align_robust(self, img1, img2, offsets0, levels=4, want_levels=False, **opts):
        """photometric alignment with a gain / bias model and Huber weights (hnet_op_photo_align_robust): as op_photo_align_pyramid; opts: the fields
        of hnet_photo_align_opts and brightness (0 / 1), huber_k (grey levels, 0: quadratic), gain0, bias0 -> records [n] of
        _capi.PHOTO_ROBUST_DTYPE; want_levels: (those, every level's records [n, levels], index = level)"""
        a = np.ascontiguousarray(img1, dtype=np.uint8).reshape(-1, IMG_H, IMG_W)
        b = np.ascontiguousarray(img2, dtype=np.uint8).reshape(-1, IMG_H, IMG_W)
        n = a.shape[0]
        if b.shape[0] != n:
            raise ValueError("img1 and img2 must hold the same number of frames")
        off = np.ascontiguousarray(offsets0, dtype=np.float32).reshape(n, 8)
        o = _capi.photo_robust_opts(**opts)
        out = np.zeros(n, _capi.PHOTO_ROBUST_DTYPE)
        lv = np.zeros((n, max(int(levels), 1)), _capi.PHOTO_ROBUST_DTYPE) if want_levels else None
        check(self._h, self._L.hnet_op_photo_align_robust(self._h, a.ctypes.data, b.ctypes.data, n, off.ctypes.data, C.addressof(o), int(levels),
                                                          out.ctypes.data, lv.ctypes.data if want_levels else None))
        return (out, lv) if want_levels else out

    def op_photo_align_masked(self, img1, mask1, img2, offsets0, levels=4, want_levels=False, **opts):
        """op_photo_align_robust on the template pixels a mask admits (hnet_op_photo_align_masked): mask1 uint8 [n, 224, 320] beside img1, non-zero = the
        pixel takes part; a mask without a zero byte gives op_photo_align_robust's records byte for byte"""
        a = np.ascontiguousarray(img1, dtype=np.uint8).reshape(-1, IMG_H, IMG_W)
        m = np.ascontiguousarray(mask1, dtype=np.uint8).reshape(-1, IMG_H, IMG_W)
        b = np.ascontiguousarray(img2, dtype=np.uint8).reshape(-1, IMG_H, IMG_W)
        n = a.shape[0]
        if b.shape[0] != n or m.shape[0] != n:
            raise ValueError("img1, mask1 and img2 must hold the same number of frames")
        off = np.ascontiguousarray(offsets0, dtype=np.float32).reshape(n, 8)
        o = _capi.photo_robust_opts(**opts)
        out = np.zeros(n, _capi.PHOTO_ROBUST_DTYPE)
        lv = np.zeros((n, max(int(levels), 1)), _capi.PHOTO_ROBUST_DTYPE) if want_levels else None
        check(self._h, self._L.hnet_op_photo_align_masked(self._h, a.ctypes.data, m.ctypes.data, b.ctypes.data, n, off.ctypes.data, C.addressof(o), int(levels),
                                                          out.ctypes.data, lv.ctypes.data if want_levels else None))
        return (out, lv) if want_levels else out

    def op_photo_search(self, img1, img2, want_scores=False, **opts):
        """coarse search over integer translations between the 40 x 28 thumbnails of uint8 frames [n, 224, 320] (hnet_op_photo_search): a start for the
        alignments from up to 240 x 160 px away; opts as _capi.photo_search_opts -> records [n] of _capi.PHOTO_SEARCH_DTYPE; want_scores: (those, the
        score of every shift [n, 41, 61], index [dy + 20, dx + 30], NaN where a shift is not scored or lies outside the radii)"""
        a = np.ascontiguousarray(img1, dtype=np.uint8).reshape(-1, IMG_H, IMG_W)
        b = np.ascontiguousarray(img2, dtype=np.uint8).reshape(-1, IMG_H, IMG_W)
        n = a.shape[0]
        if b.shape[0] != n:
            raise ValueError("img1 and img2 must hold the same number of frames")
        o = _capi.photo_search_opts(**opts)
        out = np.zeros(n, _capi.PHOTO_SEARCH_DTYPE)
        sc = np.zeros((n, _capi.PS_SHIFTS_Y, _capi.PS_SHIFTS_X)) if want_scores else None
        check(self._h, self._L.hnet_op_photo_search(self._h, a.ctypes.data, b.ctypes.data, n, C.addressof(o), out.ctypes.data,
                                                    sc.ctypes.data if want_scores else None))
        return (out, sc) if want_scores else out

    def op_keyframe_render(self, images, entries, h_origin_view, width, height, mode=_capi.RENDER_FEWEST_LINKS):
        """m (1 .. 8) stored keyframes [m, 224, 320] uint8 with their entries [m] of _capi.KEYFRAME_MAP_ENTRY_DTYPE rendered into the view h_origin_view
        [3, 3] of width x height pixels (hnet_op_keyframe_render) -> (image [height, width] uint8, cover [height, width] uint8, record [1] of
        _capi.KEYFRAME_RENDER_DTYPE); mode: _capi.RENDER_*"""
        img = np.ascontiguousarray(images, dtype=np.uint8).reshape(-1, IMG_H, IMG_W)
        ent = np.ascontiguousarray(entries, dtype=_capi.KEYFRAME_MAP_ENTRY_DTYPE).reshape(-1)
        if len(ent) != img.shape[0]:
            raise ValueError("images and entries must hold the same number of keyframes")
        hv = np.ascontiguousarray(h_origin_view, dtype=np.float64).reshape(9)
        o = _capi.KeyframeRenderOpts(int(width), int(height), int(mode), 0)
        shape = (max(int(height), 1), max(int(width), 1))
        out, cover, rec = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8), np.zeros(1, _capi.KEYFRAME_RENDER_DTYPE)
        check(self._h, self._L.hnet_op_keyframe_render(self._h, len(ent), img.ctypes.data, ent.ctypes.data, hv.ctypes.data, C.addressof(o), out.ctypes.data,
                                                       cover.ctypes.data, rec.ctypes.data))
        return out, cover, rec

    def op_keyframe_localise(self, images, entries, h_origin_pred, curr, want_images=False, **opts):
        """a camera localised against its rendered keyframe map (hnet_op_keyframe_localise): m (1 .. 8) stored keyframes [m, 224, 320] uint8 with their
        entries [m], the view h_origin_pred [3, 3] the chain predicts for the current frame and that frame curr [224, 320] -> record [1] of
        _capi.KEYFRAME_LOCALISE_DTYPE; want_images: (that, template [224, 320], cover [224, 320]); opts as _capi.keyframe_localise_opts"""
        img = np.ascontiguousarray(images, dtype=np.uint8).reshape(-1, IMG_H, IMG_W)
        ent = np.ascontiguousarray(entries, dtype=_capi.KEYFRAME_MAP_ENTRY_DTYPE).reshape(-1)
        if len(ent) != img.shape[0]:
            raise ValueError("images and entries must hold the same number of keyframes")
        hv = np.ascontiguousarray(h_origin_pred, dtype=np.float64).reshape(9)
        cur = np.ascontiguousarray(curr, dtype=np.uint8).reshape(IMG_H, IMG_W)
        o = _capi.keyframe_localise_opts(**opts)
        out = np.zeros(1, _capi.KEYFRAME_LOCALISE_DTYPE)
        tmpl, cover = np.zeros((IMG_H, IMG_W), np.uint8), np.zeros((IMG_H, IMG_W), np.uint8)
        check(self._h, self._L.hnet_op_keyframe_localise(self._h, len(ent), img.ctypes.data, ent.ctypes.data, hv.ctypes.data, cur.ctypes.data, C.addressof(o),
                                                         out.ctypes.data, tmpl.ctypes.data if want_images else None, cover.ctypes.data if want_images else None))
        return (out, tmpl, cover) if want_images else out

    def op_keyframe_adjust_solve(self, entries, edges, edge_infos=None, **opts):
        """the solve of a keyframe map's joint adjustment alone (hnet_op_keyframe_adjust_solve): entries [m] (1 .. 8) of _capi.KEYFRAME_MAP_ENTRY_DTYPE,
        edges [n_edges] (0 .. 28) of _capi.KEYFRAME_ADJUST_EDGE_DTYPE, edge_infos None or [n_edges, 8, 8] -> record [1] of _capi.KEYFRAME_ADJUST_DTYPE;
        opts as _capi.keyframe_adjust_opts"""
        ent = np.ascontiguousarray(entries, dtype=_capi.KEYFRAME_MAP_ENTRY_DTYPE).reshape(-1)
        ed = np.ascontiguousarray(edges, dtype=_capi.KEYFRAME_ADJUST_EDGE_DTYPE).reshape(-1)
        inf = None if edge_infos is None else np.ascontiguousarray(edge_infos, dtype=np.float64).reshape(len(ed), 64)
        o = _capi.keyframe_adjust_opts(**opts)
        rec = np.zeros(1, _capi.KEYFRAME_ADJUST_DTYPE)
        check(self._h, self._L.hnet_op_keyframe_adjust_solve(self._h, len(ent), ent.ctypes.data, len(ed), ed.ctypes.data if len(ed) else None,
                                                             inf.ctypes.data if inf is not None and len(ed) else None, C.addressof(o), rec.ctypes.data))
        return rec

    def op_keyframe_adjust(self, images, entries, want_edge_records=False, **opts):
        """the joint adjustment of m (1 .. 8) stored keyframes [m, 224, 320] uint8 with their entries [m] (hnet_op_keyframe_adjust): every overlapping
        pair aligned, all places solved for at once -> record [1] of _capi.KEYFRAME_ADJUST_DTYPE; want_edge_records: (that, the jobs' level-0
        alignment records [28] of _capi.PHOTO_ROBUST_DTYPE in job order); opts as _capi.keyframe_adjust_opts"""
        img = np.ascontiguousarray(images, dtype=np.uint8).reshape(-1, IMG_H, IMG_W)
        ent = np.ascontiguousarray(entries, dtype=_capi.KEYFRAME_MAP_ENTRY_DTYPE).reshape(-1)
        if len(ent) != img.shape[0]:
            raise ValueError("images and entries must hold the same number of keyframes")
        o = _capi.keyframe_adjust_opts(**opts)
        rec = np.zeros(1, _capi.KEYFRAME_ADJUST_DTYPE)
        er = np.zeros(_capi.ADJ_MAX_EDGES, _capi.PHOTO_ROBUST_DTYPE) if want_edge_records else None
        check(self._h, self._L.hnet_op_keyframe_adjust(self._h, len(ent), img.ctypes.data, ent.ctypes.data, C.addressof(o), rec.ctypes.data,
                                                       er.ctypes.data if want_edge_records else None))
        return (rec, er) if want_edge_records else rec

    def op_photo_search_oriented(self, img1, img2, hyps=None, want_scores=False, **opts):
        """the coarse search under a table of orientation hypotheses (hnet_op_photo_search_oriented): a start for the alignments for a camera that has also
        turned; hyps [n_hyp] of _capi.PHOTO_SEARCH_HYP_DTYPE (None: the default table, 60 yaws of 6 degrees), opts as _capi.photo_search_opts ->
        records [n] of _capi.PHOTO_SEARCH_ORIENTED_DTYPE; want_scores: (those, the score of every entry and shift [n, n_hyp, 41, 61])"""
        a = np.ascontiguousarray(img1, dtype=np.uint8).reshape(-1, IMG_H, IMG_W)
        b = np.ascontiguousarray(img2, dtype=np.uint8).reshape(-1, IMG_H, IMG_W)
        n = a.shape[0]
        if b.shape[0] != n:
            raise ValueError("img1 and img2 must hold the same number of frames")
        o = _capi.photo_search_opts(**opts)
        h = _capi.photo_search_table(hyps)
        out = np.zeros(n, _capi.PHOTO_SEARCH_ORIENTED_DTYPE)
        sc = np.zeros((n, max(len(h), 1), _capi.PS_SHIFTS_Y, _capi.PS_SHIFTS_X)) if want_scores else None
        check(self._h, self._L.hnet_op_photo_search_oriented(self._h, a.ctypes.data, b.ctypes.data, n, C.addressof(o), h.ctypes.data, len(h), out.ctypes.data,
                                                             sc.ctypes.data if want_scores else None))
        return (out, sc) if want_scores else out

    def op_photo_search_fine(self, img1, img2, hyps=None, fine=None, fine_opts=None, want_scores=False, **opts):
        """the oriented search followed by the fine stage around its winner on level-2 thumbnails (hnet_op_photo_search_fine): a closer start for the
        alignments, also under a coarser table; hyps as op_photo_search_oriented, fine [n_hyp, n_fine] of _capi.PHOTO_SEARCH_HYP_DTYPE (None: the table
        that matches hyps, _capi.photo_search_fine_table), fine_opts a dict of radius / n_fine / min_score, opts as _capi.photo_search_opts ->
        records [n] of _capi.PHOTO_SEARCH_FINE_DTYPE; want_scores: (those, the fine score of every entry and shift [n, n_fine, 9, 9])"""
        a = np.ascontiguousarray(img1, dtype=np.uint8).reshape(-1, IMG_H, IMG_W)
        b = np.ascontiguousarray(img2, dtype=np.uint8).reshape(-1, IMG_H, IMG_W)
        n = a.shape[0]
        if b.shape[0] != n:
            raise ValueError("img1 and img2 must hold the same number of frames")
        o = _capi.photo_search_opts(**opts)
        fo = _capi.photo_search_fine_opts(**(fine_opts or {}))
        h = _capi.photo_search_table(hyps)
        f = _capi.photo_search_fine_table(fine, hyps, fo.n_fine)
        out = np.zeros(n, _capi.PHOTO_SEARCH_FINE_DTYPE)
        sc = np.zeros((n, max(fo.n_fine, 1), _capi.PSF_SHIFTS, _capi.PSF_SHIFTS)) if want_scores else None
        check(self._h, self._L.hnet_op_photo_search_fine(self._h, a.ctypes.data, b.ctypes.data, n, C.addressof(o), h.ctypes.data, len(h), C.addressof(fo),
                                                         f.ctypes.data, out.ctypes.data, sc.ctypes.data if want_scores else None))
        return (out, sc) if want_scores else out

    def op_photo_pyramid(self, img):
        """levels 1 .. 3 of uint8 frames [n, 224, 320] (hnet_op_photo_pyramid) -> uint8 [n, _capi.PHOTO_PYRAMID_BYTES]: 160 x 112, 80 x 56 and
        40 x 28 pixels per frame, level 1 first"""
        a = np.ascontiguousarray(img, dtype=np.uint8).reshape(-1, IMG_H, IMG_W)
        out = np.zeros((a.shape[0], _capi.PHOTO_PYRAMID_BYTES), np.uint8)
        check(self._h, self._L.hnet_op_photo_pyramid(self._h, a.ctypes.data, a.shape[0], out.ctypes.data))
        return out

    def last_photo_align_device_ms(self):
        """device time of the launch sequence of the last alignment call on this context (operator or sessions), milliseconds"""
        return float(self._L.hnet_last_photo_align_device_ms(self._h))

    def op_conv(self, layer, x):
        from .weights import CONV_LAYERS
        x = np.ascontiguousarray(x, dtype=np.float32)
        b, cin, h, w = x.shape
        _n, lcin, cout, k, s = CONV_LAYERS[layer]
        assert cin == lcin
        p = (k - 1) // 2
        ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        out = np.zeros((b, cout, ho, wo), np.float32)
        check(self._h, self._L.hnet_op_conv(self._h, layer, _fp(x), b, h, w, _fp(out)))
        return out

    def op_block4_fused(self, x, reverse=False):
        """the fused block_4_0 + block_4_1 kernel alone: x [B,2,224,320] -> [B,16,112,160]"""
        x = np.ascontiguousarray(x, dtype=np.float32)
        b = x.shape[0]
        assert x.shape[1:] == (2, IMG_H, IMG_W)
        out = np.zeros((b, 16, IMG_H // 2, IMG_W // 2), np.float32)
        check(self._h, self._L.hnet_op_block4_fused(self._h, _fp(x), b, int(bool(reverse)), _fp(out)))
        return out

    def op_block3_fused(self, x):
        """the fused block_3_0 + block_3_1 kernel alone (fp16-plane mode): x [B,2,112,160] -> [B,32,56,80]"""
        x = np.ascontiguousarray(x, dtype=np.float32)
        b = x.shape[0]
        assert x.shape[1:] == (2, IMG_H // 2, IMG_W // 2)
        out = np.zeros((b, 32, IMG_H // 4, IMG_W // 4), np.float32)
        check(self._h, self._L.hnet_op_block3_fused(self._h, _fp(x), b, _fp(out)))
        return out

    def op_block42_fused(self, x):
        """the fused block_4_2 + block_4_3 kernel alone (fp16-plane mode): x [B,16,112,160] -> [B,64,28,40]"""
        x = np.ascontiguousarray(x, dtype=np.float32)
        b = x.shape[0]
        assert x.shape[1:] == (16, IMG_H // 2, IMG_W // 2)
        out = np.zeros((b, 64, IMG_H // 8, IMG_W // 8), np.float32)
        check(self._h, self._L.hnet_op_block42_fused(self._h, _fp(x), b, _fp(out)))
        return out

    def op_prep(self, img1, img2, h, k):
        i1 = np.ascontiguousarray(img1, dtype=np.float32).reshape(IMG_H, IMG_W)
        i2 = np.ascontiguousarray(img2, dtype=np.float32).reshape(IMG_H, IMG_W)
        hm = None if h is None else np.ascontiguousarray(h, dtype=np.float32).reshape(9)
        out = np.zeros((2, IMG_H // k, IMG_W // k), np.float32)
        check(self._h, self._L.hnet_op_prep(self._h, _fp(i1), _fp(i2), _fp(hm) if hm is not None else None, k, _fp(out)))
        return out

    # ---- image pre-processing (CamBase.h:165-186)
    def set_camera(self, k, d, raw_rows, raw_cols, fisheye=True):
        cam = _capi.Camera(int(bool(fisheye)), int(raw_rows), int(raw_cols), (C.c_double * 4)(*[float(x) for x in k]),
                           (C.c_double * 4)(*[float(x) for x in d]))
        check(self._h, self._L.hnet_set_camera(self._h, C.byref(cam)))

    def set_undistort_maps(self, map_x, map_y, raw_rows, raw_cols):
        mx = np.ascontiguousarray(map_x, dtype=np.float32).reshape(IMG_H, IMG_W)
        my = np.ascontiguousarray(map_y, dtype=np.float32).reshape(IMG_H, IMG_W)
        check(self._h, self._L.hnet_set_undistort_maps(self._h, _fp(mx), _fp(my), int(raw_rows), int(raw_cols)))

    def get_undistort_maps(self):
        mx, my = np.zeros((IMG_H, IMG_W), np.float32), np.zeros((IMG_H, IMG_W), np.float32)
        check(self._h, self._L.hnet_get_undistort_maps(self._h, _fp(mx), _fp(my)))
        return mx, my

    def push_raw_image(self, raw, time_stamp):
        raw = np.asarray(raw)
        if raw.dtype != np.uint8 or raw.ndim != 2:
            raise ValueError("expected a 2-D uint8 image")
        if raw.strides[1] != 1:
            raw = np.ascontiguousarray(raw)
        check(self._h, self._L.hnet_push_raw_image(self._h, raw.ctypes.data, raw.shape[0], raw.shape[1], raw.strides[0], float(time_stamp)))

    def op_undistort(self, raw):
        raw = np.ascontiguousarray(raw, dtype=np.uint8)
        out = np.zeros((IMG_H, IMG_W), np.uint8)
        check(self._h, self._L.hnet_op_undistort(self._h, raw.ctypes.data, raw.shape[0], raw.shape[1], raw.strides[0], out.ctypes.data))
        return out

    def op_prep_u8(self, img1, img2, h, k):
        i1 = np.ascontiguousarray(img1, dtype=np.uint8).reshape(IMG_H, IMG_W)
        i2 = np.ascontiguousarray(img2, dtype=np.uint8).reshape(IMG_H, IMG_W)
        hm = None if h is None else np.ascontiguousarray(h, dtype=np.float32).reshape(9)
        out = np.zeros((2, IMG_H // k, IMG_W // k), np.float32)
        u8p = C.POINTER(C.c_uint8)
        check(self._h, self._L.hnet_op_prep_u8(self._h, i1.ctypes.data_as(u8p), i2.ctypes.data_as(u8p),
                                               _fp(hm) if hm is not None else None, k, _fp(out)))
        return out

    def op_prep_batch(self, img1, img2, h, k, align_off=0, want_planes=False):
        """hnet_op_prep_batch: n pairs through one launch with the context's sampler.  img1 / img2 [n, 224, 320], both uint8 or both float32; h [n, 3, 3] or
        None; the frames sit align_off bytes past a 16-byte boundary on the device -> out [n, 2, 224 / k, 320 / k].  want_planes (k = 1 with h):
        -> (out, planes) with planes [n_planes, n, B4_HP, B4_WP] uint32, the block-4 input as the launch wrote it into a buffer of _capi.B4_SENTINEL,
        and out the values the planes join to"""
        i1, i2 = np.ascontiguousarray(img1), np.ascontiguousarray(img2)
        if i1.dtype != i2.dtype or i1.dtype not in (np.uint8, np.float32):
            raise TypeError("images must both be uint8 or float32")
        fmt = PIX_U8 if i1.dtype == np.uint8 else PIX_F32
        i1, i2 = i1.reshape(-1, IMG_H, IMG_W), i2.reshape(-1, IMG_H, IMG_W)
        n = i1.shape[0]
        if i2.shape[0] != n:
            raise ValueError("img1 and img2 must hold the same number of frames")
        hm = None if h is None else np.ascontiguousarray(h, dtype=np.float32).reshape(n, 9)
        out = np.zeros((n, 2, IMG_H // k, IMG_W // k), np.float32)
        planes = None
        if want_planes:
            n_planes = {_capi.PREC_BF16: 1, _capi.PREC_F16X2: 2}.get(self.precision(), 3)
            planes = np.zeros((n_planes, n, _capi.B4_HP, _capi.B4_WP), np.uint32)
        check(self._h, self._L.hnet_op_prep_batch(self._h, i1.ctypes.data, i2.ctypes.data, fmt, _fp(hm) if hm is not None else None, n, k, int(align_off),
                                                  _fp(out), planes.ctypes.data if want_planes else None))
        return (out, planes) if want_planes else out

    def debug_layer_output(self, layer, pair=0):
        """[Cout, Ho, Wo] output of conv layer `layer` from the last forward"""
        from .weights import CONV_LAYERS
        buf = np.zeros(8 * IMG_H * IMG_W, np.float32)
        check(self._h, self._L.hnet_debug_layer_output(self._h, layer, pair, _fp(buf), buf.size))
        h, w = {1: (28, 40), 2: (56, 80), 3: (112, 160), 4: (224, 320)}[int(CONV_LAYERS[layer][0][6])]
        for name, _cin, cout, k, s in CONV_LAYERS:
            if name[6] != CONV_LAYERS[layer][0][6]:
                continue
            p = (k - 1) // 2
            h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
            if name == CONV_LAYERS[layer][0]:
                return buf[: cout * h * w].reshape(cout, h, w).copy()
        raise AssertionError

    def debug_h_part1(self, pair=0):
        out = np.zeros(9, np.float32)
        check(self._h, self._L.hnet_debug_h_part1(self._h, pair, _fp(out)))
        return out.reshape(3, 3)


class HnetGroup:
    """hnet_group (include/hnet.h): n_ctx contexts of one configuration for INDEPENDENT steps - step k runs on member k mod n_ctx, each member on its own HIP
    stream (created first, each on its own priority level / hardware queue).  `weights`: an HNETW001 blob (bytes) or a path."""

    def __init__(self, weights, n_ctx, variant="full", mc_samples=16, dropout_p=0.05, mc_seed=0, max_batch=1, emit_error_map=False, device_id=0, precision=None):
        L = lib()
        cfg = make_config(variant, mc_samples, dropout_p, mc_seed, max_batch, emit_error_map, device_id, None, precision)
        self._L, self._g, self.variant = L, C.c_void_p(), variant
        if isinstance(weights, (bytes, bytearray)):
            buf = (C.c_char * len(weights)).from_buffer_copy(weights)
            rc = L.hnet_create_group_from_memory(C.byref(cfg), C.cast(buf, C.c_void_p), len(weights), int(n_ctx), C.byref(self._g))
        else:
            rc = L.hnet_create_group(C.byref(cfg), str(weights).encode(), int(n_ctx), C.byref(self._g))
        check(None, rc)
        self.n = int(L.hnet_group_size(self._g))
        self.members = [HnetEngine._borrow(L.hnet_group_context(self._g, i), variant) for i in range(self.n)]

    def _check(self, rc):
        if rc != _capi.HNET_OK:
            raise HnetError(rc, self._L.hnet_status_string(rc).decode() + ": " + self._L.hnet_group_last_error(self._g).decode())

    def stream(self, i):
        """member i's hipStream_t as an integer handle (torch.cuda.ExternalStream(handle) wraps it)"""
        return int(self._L.hnet_group_stream(self._g, i) or 0)

    def infer_batch_packed_device(self, d_prev, d_curr, fmt, d_prior, batch, pair_seq0, d_out72, d_err=None):
        """the next step, on the next member's stream; returns that member's index.  Does not synchronise; consecutive steps need distinct output buffers"""
        m = C.c_int(-1)
        self._check(self._L.hnet_group_infer_batch_packed_device(self._g, d_prev, d_curr, fmt, d_prior, batch, pair_seq0, d_out72, d_err, C.byref(m)))
        return int(m.value)

    def join(self, stream):
        """`stream` (a torch stream or a raw handle) waits for everything enqueued on the members so far"""
        self._check(self._L.hnet_group_join(self._g, HnetEngine._stream(stream)))

    def synchronize(self):
        self._check(self._L.hnet_group_synchronize(self._g))

    def overflow_flag(self):
        v = C.c_int(0)
        self._check(self._L.hnet_group_overflow_flag(self._g, C.byref(v)))
        return int(v.value)

    def close(self):
        if getattr(self, "_g", None):
            for m in self.members:
                m.close()
            self._L.hnet_destroy_group(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HnetSessions:
    """hnet_sessions (include/hnet.h): n_sessions camera streams on ONE context - per session its own frame ring, image count, time stamp, mask sequence
    number and undistort camera; infer() runs the current pairs of any subset as one batched forward.  Session i's result is that of a dedicated context
    driven by push_image / push_raw_image + infer.  Holds a reference to `engine`, so the context outlives the sessions."""

    def __init__(self, engine, n_sessions):
        self.engine, self._L, self.n = engine, engine._L, int(n_sessions)
        self.iter_engine = None
        self._s = C.c_void_p()
        check(engine.handle, self._L.hnet_create_sessions(engine.handle, self.n, C.byref(self._s)))
        self.emit_error_map = bool(engine.config().emit_error_map)

    def _check(self, rc):
        check(self.engine.handle, rc)

    @staticmethod
    def _ids(ids):
        ids = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.int32)
        return ids, len(ids)

    @staticmethod
    def _times(t, n):
        if t is None:
            return None
        return np.ascontiguousarray(np.broadcast_to(np.asarray(t, dtype=np.float64), (n,)))

    def push(self, ids, frames, t=None):
        """frames [n, 224, 320] uint8 (any row / frame stride with unit pixel stride) -> sessions ids; t: n time stamps or None"""
        ids, n = self._ids(ids)
        f = np.asarray(frames)
        if f.ndim == 2:
            f = f[None]
        if f.dtype != np.uint8 or f.shape[1:] != (IMG_H, IMG_W) or f.shape[0] != n:
            raise ValueError("expected frames of shape [n, 224, 320] uint8")
        if f.strides[2] != 1:
            f = np.ascontiguousarray(f)
        tt = self._times(t, n)
        self._check(self._L.hnet_sessions_push(self._s, n, ids.ctypes.data, f.ctypes.data, f.strides[1], f.strides[0],
                                               tt.ctypes.data if tt is not None else None))

    def add_camera(self, k, d, raw_rows, raw_cols, fisheye=True):
        """one more undistort camera (maps as HnetEngine.set_camera builds them); returns its index"""
        cam = _capi.Camera(int(bool(fisheye)), int(raw_rows), int(raw_cols), (C.c_double * 4)(*[float(x) for x in k]),
                           (C.c_double * 4)(*[float(x) for x in d]))
        out = C.c_int(-1)
        self._check(self._L.hnet_sessions_add_camera(self._s, C.byref(cam), C.byref(out)))
        return int(out.value)

    def bind_camera(self, id, cam):
        self._check(self._L.hnet_sessions_bind_camera(self._s, int(id), int(cam)))

    def push_raw(self, ids, raw, t=None):
        """raw [n, rows, cols] uint8: remapped with each session's camera into its ring"""
        ids, n = self._ids(ids)
        r = np.asarray(raw)
        if r.ndim == 2:
            r = r[None]
        if r.dtype != np.uint8 or r.ndim != 3 or r.shape[0] != n:
            raise ValueError("expected raw frames of shape [n, rows, cols] uint8")
        if r.strides[2] != 1:
            r = np.ascontiguousarray(r)
        tt = self._times(t, n)
        self._check(self._L.hnet_sessions_push_raw(self._s, n, ids.ctypes.data, r.ctypes.data, r.shape[1], r.shape[2], r.strides[1], r.strides[0],
                                                   tt.ctypes.data if tt is not None else None))

    def set_iterative_model(self, engine):
        """hnet_sessions_set_iterative_model: `engine` (an HnetEngine of the iterative weight file) runs IEKF iterations > 0 of infer() and of the
        filters' steps, on this object's frames; None detaches.  A reference to the engine is held while it is attached."""
        if engine is not None and not isinstance(engine, HnetEngine):
            raise TypeError("set_iterative_model expects an HnetEngine or None")
        self._check(self._L.hnet_sessions_set_iterative_model(self._s, engine.handle if engine is not None else None))
        self.iter_engine = engine

    def infer(self, ids, prior=None, want_err=False, iteration=0):
        """-> (mean [n, 8], cov [n, 8, 8][, err [n, 224, 320] uint8]); prior [n, 8] pixels (float64 as the C ABI takes it).
        iteration > 0: the IEKF re-run, on the iterative model if one is attached (hnet_sessions_infer_iter)"""
        if isinstance(iteration, bool) or not isinstance(iteration, (int, np.integer)) or iteration < 0:
            raise ValueError("iteration must be an integer >= 0")
        ids, n = self._ids(ids)
        mean = np.zeros((n, 8), np.float32)
        cov = np.zeros((n, 8, 8), np.float32)
        err = np.zeros((n, IMG_H, IMG_W), np.uint8) if want_err else None
        pr = None if prior is None else np.ascontiguousarray(prior, dtype=np.float64).reshape(n, 8)
        args = (n, ids.ctypes.data, pr.ctypes.data if pr is not None else None, mean.ctypes.data, cov.ctypes.data, err.ctypes.data if want_err else None)
        if iteration == 0:
            self._check(self._L.hnet_sessions_infer(self._s, *args))
        else:
            self._check(self._L.hnet_sessions_infer_iter(self._s, int(iteration), *args))
        return (mean, cov, err) if want_err else (mean, cov)

    def photo_residual(self, ids, offsets):
        """photometric residual records of the listed sessions' current pairs under offsets [n, m, 8] pixels -> [n, m] of _capi.PHOTO_RESIDUAL_DTYPE;
        read-only (hnet_sessions_photo_residual)"""
        ids, n = self._ids(ids)
        off = np.ascontiguousarray(offsets, dtype=np.float32).reshape(n, -1, 8)
        out = np.zeros((n, off.shape[1]), _capi.PHOTO_RESIDUAL_DTYPE)
        self._check(self._L.hnet_sessions_photo_residual(self._s, n, ids.ctypes.data, _fp(off), off.shape[1], out.ctypes.data))
        return out

    def photo_align(self, ids, offsets0, **opts):
        """photometric alignment of the listed sessions' current pairs from offsets0 [n, 8] pixels -> [n] of _capi.PHOTO_ALIGN_DTYPE; read-only
        (hnet_sessions_photo_align); opts as HnetEngine.op_photo_align"""
        ids, n = self._ids(ids)
        off = np.ascontiguousarray(offsets0, dtype=np.float32).reshape(n, 8)
        o = _capi.photo_align_opts(**opts)
        out = np.zeros(n, _capi.PHOTO_ALIGN_DTYPE)
        self._check(self._L.hnet_sessions_photo_align(self._s, n, ids.ctypes.data, off.ctypes.data, C.addressof(o), out.ctypes.data))
        return out

    def photo_align_pyramid(self, ids, offsets0, levels=4, want_levels=False, **opts):
        """coarse-to-fine photometric alignment of the listed sessions' current pairs (hnet_sessions_photo_align_pyramid); read-only; arguments and
        result as HnetEngine.op_photo_align_pyramid"""
        ids, n = self._ids(ids)
        off = np.ascontiguousarray(offsets0, dtype=np.float32).reshape(n, 8)
        o = _capi.photo_align_opts(**opts)
        out = np.zeros(n, _capi.PHOTO_ALIGN_DTYPE)
        lv = np.zeros((n, max(int(levels), 1)), _capi.PHOTO_ALIGN_DTYPE) if want_levels else None
        self._check(self._L.hnet_sessions_photo_align_pyramid(self._s, n, ids.ctypes.data, off.ctypes.data, C.addressof(o), int(levels), out.ctypes.data,
                                                              lv.ctypes.data if want_levels else None))
        return (out, lv) if want_levels else out

    def photo_align_robust(self, ids, offsets0, levels=4, want_levels=False, **opts):
        """gain / bias + Huber photometric alignment of the listed sessions' current pairs (hnet_sessions_photo_align_robust); read-only; arguments
        and result as HnetEngine.op_photo_align_robust"""
        ids, n = self._ids(ids)
        off = np.ascontiguousarray(offsets0, dtype=np.float32).reshape(n, 8)
        o = _capi.photo_robust_opts(**opts)
        out = np.zeros(n, _capi.PHOTO_ROBUST_DTYPE)
        lv = np.zeros((n, max(int(levels), 1)), _capi.PHOTO_ROBUST_DTYPE) if want_levels else None
        self._check(self._L.hnet_sessions_photo_align_robust(self._s, n, ids.ctypes.data, off.ctypes.data, C.addressof(o), int(levels), out.ctypes.data,
                                                             lv.ctypes.data if want_levels else None))
        return (out, lv) if want_levels else out

    def enable_keyframes(self):
        """hnet_sessions_enable_keyframes: allocates the keyframe store; once"""
        self._check(self._L.hnet_sessions_enable_keyframes(self._s))

    def keyframe_track(self, ids, step_px=None, **opts):
        """hnet_sessions_keyframe_track: the listed sessions' current frames against their keyframes, started from their state composed with step_px
        [n, 8] (prev -> curr offsets; None: no motion) -> [n] of _capi.KEYFRAME_TRACK_DTYPE; opts as _capi.keyframe_opts"""
        ids, n = self._ids(ids)
        step = None if step_px is None else np.ascontiguousarray(step_px, dtype=np.float32).reshape(n, 8)
        o = _capi.keyframe_opts(**opts)
        out = np.zeros(n, _capi.KEYFRAME_TRACK_DTYPE)
        self._check(self._L.hnet_sessions_keyframe_track(self._s, n, ids.ctypes.data, step.ctypes.data if step is not None else None, C.addressof(o),
                                                         out.ctypes.data))
        return out

    def keyframe_reset(self, id):
        self._check(self._L.hnet_sessions_keyframe_reset(self._s, int(id)))

    def keyframe(self, id):
        """the session's keyframe as the store holds it (hnet_sessions_get_keyframe)"""
        out = np.zeros((IMG_H, IMG_W), np.uint8)
        self._check(self._L.hnet_sessions_get_keyframe(self._s, int(id), out.ctypes.data))
        return out

    def last_keyframe_device_ms(self):
        return float(self._L.hnet_sessions_last_keyframe_device_ms(self._s))

    def enable_keyframe_map(self, capacity):
        """hnet_sessions_enable_keyframe_map: every keyframe a track takes is kept in one of `capacity` (2 .. 8) slots per session; once, after
        enable_keyframes and before any session holds a keyframe"""
        self._check(self._L.hnet_sessions_enable_keyframe_map(self._s, int(capacity)))
        self._map_capacity = int(capacity)

    def keyframe_revisit(self, ids, **opts):
        """hnet_sessions_keyframe_revisit: the listed sessions' current frames against the stored keyframe with the fewest chain links that is still in
        view; a session whose alignment passes is re-attached to it -> [n] of _capi.KEYFRAME_REVISIT_DTYPE; opts as _capi.keyframe_revisit_opts"""
        ids, n = self._ids(ids)
        o = _capi.keyframe_revisit_opts(**opts)
        out = np.zeros(n, _capi.KEYFRAME_REVISIT_DTYPE)
        self._check(self._L.hnet_sessions_keyframe_revisit(self._s, n, ids.ctypes.data, C.addressof(o), out.ctypes.data))
        return out

    def keyframe_map_info(self, id):
        """-> (entries [capacity] of _capi.KEYFRAME_MAP_ENTRY_DTYPE, map state [1] of _capi.KEYFRAME_MAP_STATE_DTYPE) of the session
        (hnet_sessions_keyframe_map_info)"""
        cap = getattr(self, "_map_capacity", _capi.KEYFRAME_MAP_MAX_CAPACITY)
        entries, state = np.zeros(cap, _capi.KEYFRAME_MAP_ENTRY_DTYPE), np.zeros(1, _capi.KEYFRAME_MAP_STATE_DTYPE)
        self._check(self._L.hnet_sessions_keyframe_map_info(self._s, int(id), entries.ctypes.data, state.ctypes.data))
        return entries, state

    def map_keyframe(self, id, slot):
        """the image in slot `slot` of the session's map as the store holds it (hnet_sessions_get_map_keyframe)"""
        out = np.zeros((IMG_H, IMG_W), np.uint8)
        self._check(self._L.hnet_sessions_get_map_keyframe(self._s, int(id), int(slot), out.ctypes.data))
        return out

    def enable_keyframe_render(self, max_width, max_height):
        """hnet_sessions_enable_keyframe_render: allocates the render's buffers for views up to max_width x max_height; once, after enable_keyframe_map"""
        self._check(self._L.hnet_sessions_enable_keyframe_render(self._s, int(max_width), int(max_height)))

    def keyframe_render(self, ids, width, height, h_origin_view=None, mode=_capi.RENDER_FEWEST_LINKS):
        """hnet_sessions_keyframe_render: the listed sessions' keyframe maps, each into its view h_origin_view [n, 3, 3] (None: each session's current
        frame as its origin chain predicts it) of width x height pixels -> (images [n, height, width] uint8, covers [n, height, width] uint8, records
        [n] of _capi.KEYFRAME_RENDER_DTYPE); read-only; mode: _capi.RENDER_*"""
        ids, n = self._ids(ids)
        hv = None if h_origin_view is None else np.ascontiguousarray(h_origin_view, dtype=np.float64).reshape(n, 9)
        o = _capi.KeyframeRenderOpts(int(width), int(height), int(mode), 0)
        shape = (n, max(int(height), 1), max(int(width), 1))
        out, cover, rec = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8), np.zeros(n, _capi.KEYFRAME_RENDER_DTYPE)
        self._check(self._L.hnet_sessions_keyframe_render(self._s, n, ids.ctypes.data, hv.ctypes.data if hv is not None else None, C.addressof(o),
                                                          out.ctypes.data, cover.ctypes.data, rec.ctypes.data))
        return out, cover, rec

    def enable_keyframe_localise(self):
        """hnet_sessions_enable_keyframe_localise: allocates the localise's templates, masks, tables and records; once, after enable_keyframe_map"""
        self._check(self._L.hnet_sessions_enable_keyframe_localise(self._s))

    def keyframe_localise(self, ids, **opts):
        """hnet_sessions_keyframe_localise: each listed session's current frame localised against its rendered keyframe map -> records [n] of
        _capi.KEYFRAME_LOCALISE_DTYPE; apply=1 corrects the chain of a LOCALISED session; opts as _capi.keyframe_localise_opts"""
        ids, n = self._ids(ids)
        o = _capi.keyframe_localise_opts(**opts)
        out = np.zeros(n, _capi.KEYFRAME_LOCALISE_DTYPE)
        self._check(self._L.hnet_sessions_keyframe_localise(self._s, n, ids.ctypes.data, C.addressof(o), out.ctypes.data))
        return out

    def enable_keyframe_adjust(self):
        """hnet_sessions_enable_keyframe_adjust: allocates the adjustment's tables, records and pinned blocks; once, after enable_keyframe_map"""
        self._check(self._L.hnet_sessions_enable_keyframe_adjust(self._s))

    def keyframe_adjust(self, ids, want_edge_records=False, **opts):
        """hnet_sessions_keyframe_adjust: the listed sessions' keyframe maps, each adjusted jointly -> records [n] of _capi.KEYFRAME_ADJUST_DTYPE;
        want_edge_records: (those, the jobs' level-0 alignment records [n, 28] of _capi.PHOTO_ROBUST_DTYPE).  apply=1 writes the new matrices into the
        maps; otherwise read-only.  opts as _capi.keyframe_adjust_opts"""
        ids, n = self._ids(ids)
        o = _capi.keyframe_adjust_opts(**opts)
        rec = np.zeros(n, _capi.KEYFRAME_ADJUST_DTYPE)
        er = np.zeros((n, _capi.ADJ_MAX_EDGES), _capi.PHOTO_ROBUST_DTYPE) if want_edge_records else None
        self._check(self._L.hnet_sessions_keyframe_adjust(self._s, n, ids.ctypes.data, C.addressof(o), rec.ctypes.data,
                                                          er.ctypes.data if want_edge_records else None))
        return (rec, er) if want_edge_records else rec

    def photo_search(self, ids, **opts):
        """coarse search over integer translations on the listed sessions' current pairs (hnet_sessions_photo_search); read-only; result as
        HnetEngine.op_photo_search"""
        ids, n = self._ids(ids)
        o = _capi.photo_search_opts(**opts)
        out = np.zeros(n, _capi.PHOTO_SEARCH_DTYPE)
        self._check(self._L.hnet_sessions_photo_search(self._s, n, ids.ctypes.data, C.addressof(o), out.ctypes.data))
        return out

    def keyframe_relocalise(self, ids, **opts):
        """hnet_sessions_keyframe_relocalise: the listed sessions' current frames searched against their held keyframe and every stored one, aligned
        against the best FOUND candidate from the searched start; a session whose alignment passes is re-tracked on its keyframe or re-attached to the
        stored one -> [n] of _capi.KEYFRAME_RELOC_DTYPE; opts as _capi.keyframe_relocalise_opts"""
        ids, n = self._ids(ids)
        o = _capi.keyframe_relocalise_opts(**opts)
        out = np.zeros(n, _capi.KEYFRAME_RELOC_DTYPE)
        self._check(self._L.hnet_sessions_keyframe_relocalise(self._s, n, ids.ctypes.data, C.addressof(o), out.ctypes.data))
        return out

    def photo_search_oriented(self, ids, hyps=None, **opts):
        """the search under a table of orientation hypotheses on the listed sessions' current pairs (hnet_sessions_photo_search_oriented); read-only;
        result as HnetEngine.op_photo_search_oriented"""
        ids, n = self._ids(ids)
        o = _capi.photo_search_opts(**opts)
        h = _capi.photo_search_table(hyps)
        out = np.zeros(n, _capi.PHOTO_SEARCH_ORIENTED_DTYPE)
        self._check(self._L.hnet_sessions_photo_search_oriented(self._s, n, ids.ctypes.data, C.addressof(o), h.ctypes.data, len(h), out.ctypes.data))
        return out

    def keyframe_relocalise_oriented(self, ids, hyps=None, **opts):
        """hnet_sessions_keyframe_relocalise_oriented: keyframe_relocalise with the search under a table of orientation hypotheses (hyps as
        op_photo_search_oriented) -> [n] of _capi.KEYFRAME_RELOC_ORIENTED_DTYPE; opts as _capi.keyframe_relocalise_opts"""
        ids, n = self._ids(ids)
        o = _capi.keyframe_relocalise_opts(**opts)
        h = _capi.photo_search_table(hyps)
        out = np.zeros(n, _capi.KEYFRAME_RELOC_ORIENTED_DTYPE)
        self._check(self._L.hnet_sessions_keyframe_relocalise_oriented(self._s, n, ids.ctypes.data, C.addressof(o), h.ctypes.data, len(h), out.ctypes.data))
        return out

    def photo_search_fine(self, ids, hyps=None, fine=None, fine_opts=None, **opts):
        """the oriented search and the fine stage on the listed sessions' current pairs (hnet_sessions_photo_search_fine); read-only; result as
        HnetEngine.op_photo_search_fine"""
        ids, n = self._ids(ids)
        o = _capi.photo_search_opts(**opts)
        fo = _capi.photo_search_fine_opts(**(fine_opts or {}))
        h = _capi.photo_search_table(hyps)
        f = _capi.photo_search_fine_table(fine, hyps, fo.n_fine)
        out = np.zeros(n, _capi.PHOTO_SEARCH_FINE_DTYPE)
        self._check(self._L.hnet_sessions_photo_search_fine(self._s, n, ids.ctypes.data, C.addressof(o), h.ctypes.data, len(h), C.addressof(fo), f.ctypes.data,
                                                            out.ctypes.data))
        return out

    def keyframe_relocalise_fine(self, ids, hyps=None, fine=None, fine_opts=None, **opts):
        """hnet_sessions_keyframe_relocalise_fine: keyframe_relocalise_oriented with the fine stage on the picked candidate, whose final start the
        alignment takes (hyps, fine and fine_opts as op_photo_search_fine) -> [n] of _capi.KEYFRAME_RELOC_FINE_DTYPE; opts as
        _capi.keyframe_relocalise_opts"""
        ids, n = self._ids(ids)
        o = _capi.keyframe_relocalise_opts(**opts)
        fo = _capi.photo_search_fine_opts(**(fine_opts or {}))
        h = _capi.photo_search_table(hyps)
        f = _capi.photo_search_fine_table(fine, hyps, fo.n_fine)
        out = np.zeros(n, _capi.KEYFRAME_RELOC_FINE_DTYPE)
        self._check(self._L.hnet_sessions_keyframe_relocalise_fine(self._s, n, ids.ctypes.data, C.addressof(o), h.ctypes.data, len(h), C.addressof(fo),
                                                                   f.ctypes.data, out.ctypes.data))
        return out

    def keyframe_track_recover(self, ids, step_px=None, hyps=None, track=None, reloc=None):
        """hnet_sessions_keyframe_track_recover: keyframe_track whose LOST sessions are relocalised (oriented; hyps as op_photo_search_oriented) before
        their re-key is committed; a recovered session keeps its keyframe or is attached to a stored one and its track record holds KF_RECOVERED, an
        unrecovered one gets keyframe_track's result -> [n] of _capi.KEYFRAME_RECOVER_DTYPE; track / reloc as _capi.keyframe_recover_opts"""
        ids, n = self._ids(ids)
        step = None if step_px is None else np.ascontiguousarray(step_px, dtype=np.float32).reshape(n, 8)
        o = _capi.keyframe_recover_opts(track, reloc)
        h = _capi.photo_search_table(hyps)
        out = np.zeros(n, _capi.KEYFRAME_RECOVER_DTYPE)
        self._check(self._L.hnet_sessions_keyframe_track_recover(self._s, n, ids.ctypes.data, step.ctypes.data if step is not None else None, C.addressof(o),
                                                                 h.ctypes.data, len(h), out.ctypes.data))
        return out

    def image_count(self, id):
        return int(self._L.hnet_sessions_image_count(self._s, int(id)))

    def latest_time(self, id):
        return float(self._L.hnet_sessions_latest_time(self._s, int(id)))

    def set_seq(self, id, seq):
        self._check(self._L.hnet_sessions_set_seq(self._s, int(id), int(seq)))

    def seq(self, id):
        return int(self._L.hnet_sessions_seq(self._s, int(id)))

    def reset(self, id):
        self._check(self._L.hnet_sessions_reset(self._s, int(id)))

    def frame(self, id, which):
        """the session's previous (0) or current (1) 224 x 320 frame as the ring holds it"""
        out = np.zeros((IMG_H, IMG_W), np.uint8)
        self._check(self._L.hnet_sessions_get_frame(self._s, int(id), int(which), out.ctypes.data))
        return out

    def last_timing(self):
        t = Timing()
        self._check(self._L.hnet_sessions_last_timing(self._s, C.byref(t)))
        return {"device_ms": t.device_ms, "host_ms": t.host_ms, "n_inferences": t.n_inferences,
                "sum_device_ms_after_100": t.sum_device_ms_after_100, "n_main_inferences": t.n_main_inferences}

    def close(self):
        if getattr(self, "_s", None):
            self._L.hnet_destroy_sessions(self._s)
            self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HnetFilters:
    """hnet_filters (include/hnet.h): one 27-state filter per session of `sessions`, stepped on the device.  step() runs, for any subset of the
    sessions, the IMU propagation, max_iekf_iteration batched forwards each followed by the filter update under the reference's gate, and the
    offsets reset, with one synchronisation; each session's result is hnet_ekf::propagate_with_imu + iterated_update around a dedicated context.
    States are numpy records of _capi.FILTER_STATE_DTYPE, IMU readings of _capi.IMU_DTYPE.  Holds a reference to `sessions`."""

    def __init__(self, sessions, max_iekf_iteration=1):
        self.sessions, self._L, self.iters = sessions, sessions._L, int(max_iekf_iteration)
        self._f = C.c_void_p()
        check(sessions.engine.handle, self._L.hnet_create_filters(sessions._s, self.iters, C.byref(self._f)))

    def _check(self, rc):
        check(self.sessions.engine.handle, rc)

    @staticmethod
    def default_params():
        p = _capi.FilterParams()
        _capi.lib().hnet_filter_default_params(C.byref(p))
        return p

    def set_params(self, id, params):
        self._check(self._L.hnet_filters_set_params(self._f, int(id), C.byref(params)))

    def set_state(self, id, state):
        st = np.ascontiguousarray(np.asarray(state, dtype=_capi.FILTER_STATE_DTYPE).reshape(()))
        self._check(self._L.hnet_filters_set_state(self._f, int(id), st.ctypes.data))

    def get_state(self, ids):
        ids = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.int32)
        out = np.zeros(len(ids), _capi.FILTER_STATE_DTYPE)
        self._check(self._L.hnet_filters_get_state(self._f, len(ids), ids.ctypes.data, out.ctypes.data))
        return out

    def step(self, ids, t_frame, imu):
        """ids [n]; t_frame [n]; imu: n arrays of IMU_DTYPE readings (session ids[i]'s window, time ordered).
        -> (states [n] FILTER_STATE_DTYPE, net [iters, n, 72] float32 (mean | cov of every forward), updates [n] int32)"""
        ids = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.int32)
        n = len(ids)
        tf = np.ascontiguousarray(np.broadcast_to(np.asarray(t_frame, dtype=np.float64), (n,)))
        if len(imu) != n:
            raise ValueError("one IMU array per session")
        parts = [np.asarray(r, dtype=_capi.IMU_DTYPE).reshape(-1) for r in imu]
        off = np.zeros(n + 1, np.int64)
        off[1:] = np.cumsum([len(r) for r in parts])
        rd = np.ascontiguousarray(np.concatenate(parts) if off[-1] else np.zeros(1, _capi.IMU_DTYPE))
        states = np.zeros(n, _capi.FILTER_STATE_DTYPE)
        net = np.zeros((self.iters, n, 72), np.float32)
        upd = np.zeros(n, np.int32)
        self._check(self._L.hnet_filters_step(self._f, n, ids.ctypes.data, tf.ctypes.data, rd.ctypes.data, off.ctypes.data, states.ctypes.data,
                                              net.ctypes.data, upd.ctypes.data))
        return states, net, upd

    # ---- the fed interface: device IMU rings, the static initialiser, one call that advances every camera that is ready ----
    @staticmethod
    def default_init_params():
        p = _capi.InitParams()
        _capi.lib().hnet_filter_default_init_params(C.byref(p))
        return p

    def enable_feed(self, imu_capacity):
        """allocates one device ring of imu_capacity readings per session (once)"""
        self._check(self._L.hnet_filters_enable_feed(self._f, int(imu_capacity)))

    def set_init_params(self, id, params):
        self._check(self._L.hnet_filters_set_init_params(self._f, int(id), C.byref(params)))

    def feed_imu(self, ids, imu):
        """ids [n]; imu: n arrays of IMU_DTYPE readings, each in non-decreasing time and not older than what the session was fed before.
        One upload, one kernel, no synchronisation."""
        ids = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.int32)
        if len(imu) != len(ids):
            raise ValueError("one IMU array per session")
        parts = [np.asarray(r, dtype=_capi.IMU_DTYPE).reshape(-1) for r in imu]
        off = np.zeros(len(ids) + 1, np.int64)
        off[1:] = np.cumsum([len(r) for r in parts])
        rd = np.ascontiguousarray(np.concatenate(parts) if off[-1] else np.zeros(1, _capi.IMU_DTYPE))
        self._check(self._L.hnet_filters_feed_imu(self._f, len(ids), ids.ctypes.data, rd.ctypes.data, off.ctypes.data))

    def initialized(self, id):
        return self._L.hnet_filters_initialized(self._f, int(id)) == 1

    def uninitialize(self, id):
        self._check(self._L.hnet_filters_uninitialize(self._f, int(id)))

    def advance(self, ids):
        """track_image_and_update for the listed sessions, on each one's latest pushed frame, with one synchronisation.
        -> (states [n] FILTER_STATE_DTYPE (rows of sessions that did not move stay zero), net [iters, n, 72] float32 (rows of STEPPED sessions),
            updates [n] int32, status [n] int32 of _capi.ADV_*)"""
        ids = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.int32)
        n = len(ids)
        states = np.zeros(n, _capi.FILTER_STATE_DTYPE)
        net = np.zeros((self.iters, n, 72), np.float32)
        upd = np.zeros(n, np.int32)
        status = np.zeros(n, np.int32)
        self._check(self._L.hnet_filters_advance(self._f, n, ids.ctypes.data, states.ctypes.data, net.ctypes.data, upd.ctypes.data, status.ctypes.data))
        return states, net, upd, status

    def last_selection(self, id):
        """the readings the last advance selected for session id (IMU_DTYPE), as hnet_ekf::select_imu_readings writes them"""
        cnt = C.c_int(0)
        self._check(self._L.hnet_filters_last_selection(self._f, int(id), None, 0, C.byref(cnt)))
        out = np.zeros(max(cnt.value, 1), _capi.IMU_DTYPE)
        self._check(self._L.hnet_filters_last_selection(self._f, int(id), out.ctypes.data, cnt.value, C.byref(cnt)))
        return out[:cnt.value]

    def predict(self, ids, t_query):
        """the listed sessions' states predicted to t_query [n] (camera clock) from the device's IMU rings, read-only, with one launch and one
        synchronisation -> [n] records of _capi.ODOMETRY_DTYPE (status: _capi.PRED_*)"""
        ids = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.int32)
        n = len(ids)
        tq = np.ascontiguousarray(np.broadcast_to(np.asarray(t_query, dtype=np.float64), (n,)))
        out = np.zeros(n, _capi.ODOMETRY_DTYPE)
        self._check(self._L.hnet_filters_predict(self._f, n, ids.ctypes.data, tq.ctypes.data, out.ctypes.data))
        return out

    def predict_cov(self, ids, t_query, full=False):
        """predict() with the covariance at the query time, read-only -> (records of _capi.ODOMETRY_DTYPE [n], records of _capi.ODOMETRY_COV_DTYPE [n])
        and, with full, the propagated 27 x 27 covariances [n, 27, 27] as a third item"""
        ids = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.int32)
        n = len(ids)
        tq = np.ascontiguousarray(np.broadcast_to(np.asarray(t_query, dtype=np.float64), (n,)))
        out = np.zeros(n, _capi.ODOMETRY_DTYPE)
        cov = np.zeros(n, _capi.ODOMETRY_COV_DTYPE)
        P = np.zeros((n, 27, 27)) if full else None
        self._check(self._L.hnet_filters_predict_cov(self._f, n, ids.ctypes.data, tq.ctypes.data, out.ctypes.data, cov.ctypes.data,
                                                     P.ctypes.data if full else None))
        return (out, cov, P) if full else (out, cov)

    def last_predict_cov_device_ms(self):
        """as last_predict_device_ms, for predict_cov"""
        return float(self._L.hnet_filters_last_predict_cov_device_ms(self._f))

    def newest_imu_time(self, id):
        """the time (IMU clock) of the newest reading session id was fed; NaN for an empty ring"""
        return float(self._L.hnet_filters_newest_imu_time(self._f, int(id)))

    def last_predict_device_ms(self):
        """event time of the last timed predict's launch; the first call switches the timing on (NaN until a timed predict has run)"""
        return float(self._L.hnet_filters_last_predict_device_ms(self._f))

    # ---- innovation records and the NIS gate ----
    def enable_innovations(self):
        """from now on every step / advance also returns one innovation record per iteration and stepping session (once per object)"""
        self._check(self._L.hnet_filters_enable_innovations(self._f))

    def set_nis_gate(self, id, max_nis):
        """session id's gate on the normalised innovation squared; 0 = off.  chi-squared with 8 degrees of freedom: 15.507 (95 %), 20.090 (99 %),
        26.124 (99.9 %)"""
        self._check(self._L.hnet_filters_set_nis_gate(self._f, int(id), float(max_nis)))

    def last_innovations(self, n):
        """the records [iters, n] of _capi.INNOVATION_DTYPE of the last step (of n sessions; another n is refused)"""
        out = np.zeros((self.iters, int(n)), _capi.INNOVATION_DTYPE)
        self._check(self._L.hnet_filters_last_innovations(self._f, int(n), out.ctypes.data))
        return out

    def innovation_stats(self, id):
        st = _capi.InnovationStats()
        self._check(self._L.hnet_filters_innovation_stats(self._f, int(id), C.byref(st)))
        return {"used": st.used, "rejected": st.rejected, "singular": st.singular, "sum_nis": st.sum_nis, "max_nis": st.max_nis}

    def reset_innovation_stats(self, id):
        self._check(self._L.hnet_filters_reset_innovation_stats(self._f, int(id)))

    # ---- photometric residual records ----
    def enable_photometric(self):
        """from now on every step / advance also returns 2 + iters photometric residual records per stepping session (once per object)"""
        self._check(self._L.hnet_filters_enable_photometric(self._f))

    def last_photometric(self, n):
        """the records [n, 2 + iters] of _capi.PHOTO_RESIDUAL_DTYPE of the last step (of n sessions; another n is refused): identity, the prior of
        iteration 0, the packed mean of every forward"""
        out = np.zeros((int(n), 2 + self.iters), _capi.PHOTO_RESIDUAL_DTYPE)
        self._check(self._L.hnet_filters_last_photometric(self._f, int(n), out.ctypes.data))
        return out

    def set_photo_gate(self, id, max_ratio, min_inside=0):
        """session id's photometric gate (needs enable_photometric): an update is refused when its estimate's mean residual inside the image exceeds
        max_ratio times the prior's, or the estimate is degenerate or has fewer than max(min_inside, 1) pixels inside; 0 = off"""
        self._check(self._L.hnet_filters_set_photo_gate(self._f, int(id), float(max_ratio), int(min_inside)))

    def photo_stats(self, id):
        st = _capi.PhotoStats()
        self._check(self._L.hnet_filters_photo_stats(self._f, int(id), C.byref(st)))
        return {"judged": st.judged, "rejected": st.rejected, "degenerate": st.degenerate, "sum_ratio": st.sum_ratio, "max_ratio": st.max_ratio}

    def reset_photo_stats(self, id):
        self._check(self._L.hnet_filters_reset_photo_stats(self._f, int(id)))

    def set_photo_gate_taps(self, from_global):
        """tools: the single-candidate launches of a gated step read img2 from global memory (True) or stage it in LDS (False); same records"""
        self._check(self._L.hnet_filters_set_photo_gate_taps(self._f, 1 if from_global else 0))

    # ---- the photometric fallback (include/hnet.h hnet_filters_set_photo_refine) ----
    def set_photo_refine(self, id, opts):
        """session id's fallback after a photometric refusal at iteration 0 (needs enable_photometric): opts from _capi.photo_refine_opts(cov_scale = ...,
        ...), None = off.  The refining sessions of one step must share the alignment options and levels"""
        self._check(self._L.hnet_filters_set_photo_refine(self._f, int(id), C.byref(opts) if opts is not None else None))

    def last_refine(self, n):
        """the records [n] of _capi.PHOTO_REFINE_DTYPE of the last step (of n sessions; another n, or a step without a refining session, is refused)"""
        out = np.zeros(int(n), _capi.PHOTO_REFINE_DTYPE)
        self._check(self._L.hnet_filters_last_refine(self._f, int(n), out.ctypes.data))
        return out

    def refine_stats(self, id):
        st = _capi.RefineStats()
        self._check(self._L.hnet_filters_refine_stats(self._f, int(id), C.byref(st)))
        return {"asked": st.asked, "applied": st.applied, "unusable": st.unusable, "nis_rejected": st.nis_rejected, "sum_nis": st.sum_nis, "max_nis": st.max_nis}

    def reset_refine_stats(self, id):
        self._check(self._L.hnet_filters_reset_refine_stats(self._f, int(id)))

    # ---- the keyframe track as an in-step measurement (include/hnet.h hnet_filters_set_keyframe_measure) ----
    def set_keyframe_measure(self, id, opts):
        """session id's keyframe track inside the step, fed to the filter before the reset (needs the sessions' enable_keyframes): opts from
        _capi.keyframe_measure_opts(cov_scale = ...), or None = off"""
        self._check(self._L.hnet_filters_set_keyframe_measure(self._f, int(id), C.byref(opts) if opts is not None else None))

    def last_keyframe_measure(self, n):
        """the records [n] of _capi.KEYFRAME_MEASURE_DTYPE of the last step (of n sessions; another n, or a step without a measuring session, is refused)"""
        out = np.zeros(int(n), _capi.KEYFRAME_MEASURE_DTYPE)
        self._check(self._L.hnet_filters_last_keyframe_measure(self._f, int(n), out.ctypes.data))
        return out

    def set_keyframe_recover(self, id, reloc=None, hyps=None):
        """recovery inside session id's in-step keyframe track (hnet_filters_set_keyframe_recover; the session must measure): reloc a KeyframeRelocOpts
        or a dict in the keyword form of _capi.keyframe_relocalise_opts, hyps as op_photo_search_oriented (None: the default yaw table); reloc None = off"""
        if reloc is None:
            self._check(self._L.hnet_filters_set_keyframe_recover(self._f, int(id), None, None, 0))
            return
        o = reloc if isinstance(reloc, _capi.KeyframeRelocOpts) else _capi.keyframe_relocalise_opts(**reloc)
        h = _capi.photo_search_table(hyps)
        self._check(self._L.hnet_filters_set_keyframe_recover(self._f, int(id), C.addressof(o), h.ctypes.data, len(h)))

    def last_keyframe_recover(self, n):
        """the records [n] of _capi.KEYFRAME_MEASURE_RECOVER_DTYPE of the last step (of n sessions; another n, or a step without a recovering session,
        is refused)"""
        out = np.zeros(int(n), _capi.KEYFRAME_MEASURE_RECOVER_DTYPE)
        self._check(self._L.hnet_filters_last_keyframe_recover(self._f, int(n), out.ctypes.data))
        return out

    def keyframe_measure_stats(self, id):
        st = _capi.KeyframeMeasureStats()
        self._check(self._L.hnet_filters_keyframe_measure_stats(self._f, int(id), C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_}

    def reset_keyframe_measure_stats(self, id):
        self._check(self._L.hnet_filters_reset_keyframe_measure_stats(self._f, int(id)))

    def last_priors(self, n):
        """the fp32 priors [iters, n, 8] the forwards of the last step (of n sessions; another n is refused) read"""
        out = np.zeros((self.iters, int(n), 8), np.float32)
        self._check(self._L.hnet_filters_last_priors(self._f, int(n), out.ctypes.data))
        return out

    def last_timing(self):
        t = Timing()
        self._check(self._L.hnet_filters_last_timing(self._f, C.byref(t)))
        return {"device_ms": t.device_ms, "host_ms": t.host_ms, "n_inferences": t.n_inferences, "n_steps": t.n_main_inferences}

    def close(self):
        if getattr(self, "_f", None):
            self._L.hnet_destroy_filters(self._f)
            self._f = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HomographyNet:
    """Mirror of ``pytorch::HomographyNet`` (HomographyNet.h:23-67).

    HomographyNet(network_model_path, network_model_iterative_path, use_prior, num_of_iteration, show_imgs)
    — the model path names an HNETW001 weight blob instead of a TorchScript file; as in the reference the
    substring "_showError" in the path selects the variant that also produces the photometric error map
    (HomographyNet.cpp:96-100).  The extra keyword arguments expose what the reference freezes at trace time.
    """

    def __init__(self, network_model_path, network_model_iterative_path="", use_prior=False, num_of_iteration=1,
                 show_imgs=False, *, blocks_to_run=None, mc_samples=None, dropout_p=None, mc_seed=0, device_id=0,
                 weights_blob=None, precision=None, blocks_to_run_iterative=None, weights_blob_iterative=None):
        """blocks_to_run / mc_samples / dropout_p = None: from the file's `hnet.variant` record (what the reference freezes into the traced .pt;
        a record-less blob gives the reference's launch values 3 / 16 / 0.05) - explicit values are overrides, as HNET_* are for the C++ adapter"""
        self.use_prior_4pt_offset = bool(use_prior)
        self.cv_imshow = bool(show_imgs)
        self.iteration = num_of_iteration > 1
        main_err, iter_err = "_showError" in str(network_model_path), "_showError" in str(network_model_iterative_path)

        def make(weights, blocks, emit):
            variant = "full" if not use_prior else (None if blocks is None else {3: "prior3", 2: "prior2", 1: "prior1"}[blocks])
            e = HnetEngine(weights, variant=variant, mc_samples=mc_samples, dropout_p=dropout_p, mc_seed=mc_seed, max_batch=1,
                           emit_error_map=emit, device_id=device_id, precision=precision)
            u = e.config()
            if bool(u.use_prior) != bool(use_prior):
                e.close()
                raise ValueError("use_prior disagrees with the variant recorded in the weight file")
            print(f"model variant: {e.variant}, MC-dropout N = {u.mc_samples}, p = {u.dropout_p:g}, error map {'on' if u.emit_error_map else 'off'}")
            return e, bool(u.emit_error_map)

        print("Loading the Network Model (HNETW001 weights) ...")
        # ("_showError" in the name forces the map like the reference's sniff; otherwise the file's record decides; unused with an iterative model, :199)
        self._eng, any_err = make(weights_blob if weights_blob is not None else network_model_path, blocks_to_run,
                                  False if self.iteration else (True if main_err else None))
        t = self._eng.last_timing()
        print(f"[TIME]: {t['host_ms']:.4f} milliseconds for the first network inference")
        self._eng_iter = None
        if self.iteration:      # HomographyNet.cpp:20-24: a second model for iteration > 0, warmed up (:49-56), fed the same frames
            w_it = weights_blob_iterative if weights_blob_iterative is not None else (weights_blob if weights_blob is not None else network_model_iterative_path)
            self._eng_iter, any_err = make(w_it, blocks_to_run_iterative, True if iter_err else None)
            check(self._eng_iter.handle, self._eng._L.hnet_attach_images(self._eng_iter.handle, self._eng.handle))
            print("IEKF! Load the Network for Iteration!")
        self.show_phtometric_error = any_err       # one member in the reference: the file loaded last decides (:96-100, :117-121)
        self._pred_mean = np.zeros((8, 1), np.float32)
        self._pred_Cov = np.zeros((8, 8), np.float32)
        self.last_error_map = None

    @property
    def img_counter(self):
        return self._eng._L.hnet_image_count(self._eng.handle)

    def load_current_img(self, img, time_stamp):
        """HomographyNet.cpp:127-151 — img: 224x320 uint8 (a cv::Mat CV_8UC1 in the reference)"""
        img = np.asarray(img)
        if img.dtype != np.uint8 or img.shape != (IMG_H, IMG_W):
            raise ValueError("expected a 224x320 uint8 image")
        if img.strides[1] != 1:
            img = np.ascontiguousarray(img)
        if self.img_counter == 0:
            print("First Image Comes into the Network Object!")
        check(self._eng.handle, self._eng._L.hnet_push_image(self._eng.handle, img.ctypes.data, IMG_H, IMG_W,
                                                              img.strides[0], float(time_stamp)))

    def network_inference(self, prior_4pt_offset_vec, num_of_inference=0):
        """HomographyNet.cpp:153-252"""
        mean = np.zeros(8, np.float32)
        cov = np.zeros((8, 8), np.float32)
        net = self._eng_iter if (self._eng_iter is not None and num_of_inference > 0) else self._eng      # HomographyNet_model / _model_iterative (:183, :211)
        err = np.zeros((IMG_H, IMG_W), np.uint8) if (self.show_phtometric_error and (net is self._eng_iter or not self.iteration)) else None
        pr = None
        if self.use_prior_4pt_offset:
            pr = np.ascontiguousarray(prior_4pt_offset_vec, dtype=np.float64).reshape(8)
        rc = self._eng._L.hnet_infer(net.handle, pr.ctypes.data_as(C.POINTER(C.c_double)) if pr is not None else None,
                                     int(num_of_inference), _fp(mean), _fp(cov),
                                     err.ctypes.data_as(C.POINTER(C.c_uint8)) if err is not None else None)
        if rc == _capi.ERR_NOT_READY:   # :155-158 prints and returns with the previous outputs
            print("HNet cannot inference! Only has one image!")
            return
        check(net.handle, rc)
        self._pred_mean = mean.reshape(8, 1)
        self._pred_Cov = cov
        self.last_error_map = err
        if num_of_inference == 0:
            t = self._eng.last_timing()
            if t["n_main_inferences"] > 100:
                avg = t["sum_device_ms_after_100"] / (t["n_main_inferences"] - 100)
                print(f"[TIME]: {t['device_ms']:.3f} (avg. = {avg:.3f}) milliseconds for pure network inference")

    def get_pred_mean(self):
        return self._pred_mean.astype(np.float64)

    def get_pred_Cov(self):
        return self._pred_Cov.astype(np.float64)

    def get_latest_inference_time(self):
        return self._eng._L.hnet_latest_time(self._eng.handle)

    def close(self):
        """the iterative model's context reads the main context's frames (hnet_attach_images): it goes first"""
        if getattr(self, "_eng_iter", None) is not None:
            self._eng_iter.close()
            self._eng_iter = None
        if getattr(self, "_eng", None) is not None:
            self._eng.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
