"""CPU: the iterative-model calls of hnet_sessions (include/hnet.h hnet_sessions_set_iterative_model, hnet_sessions_infer_iter) are exported and
refuse NULL handles; the Python wrappers validate their arguments before any call into the library; and the weight file that
tests/test_gpu_sessions_iterative.py uses for the repair path has the properties that test relies on, checked with the CPU oracle.

The repair test needs an iterative model whose activations leave the fp16-plane range while its weights stay inside it (so hnet_create keeps
HNET_PREC_F16X2 and the overflow shows up during a step).  overflow_iterative_state() builds it from the tests' synthetic weights: the seven convolutions
of block 4 (the only block prior-1 runs) are scaled by g, which grows block 4's activations by about g per layer, and the heads' Linear(5120, 256) by
g^-7, which keeps the outputs at the scale of the unscaled model.  choose_overflow_gain() picks the smallest g of OVERFLOW_GAINS for which the oracle's
forward on the test's pair has a block-4 activation feeding another convolution beyond 65504 (the fp16 maximum), every weight below the bound that
demotes at hnet_create, and finite outputs."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
FP16_MAX = 65504.0
OVERFLOW_GAINS = (8.0, 12.0, 16.0, 24.0, 32.0)
ITER_MODEL = dict(variant="prior1", mc_samples=8, dropout_p=0.1)


def _lib():
    from cuahn_vio_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _capi, _capi.lib()


def overflow_iterative_state(gain):
    """synthetic_state(0) with block 4's convolutions scaled by `gain` and the heads' Linear(5120, 256) weights by gain^-7"""
    from cuahn_vio_amd import weights
    st = weights.synthetic_state(0)
    g = np.float32(gain)
    for k in st:
        if k.startswith("model_last_block_list.0.block_4_") and k.endswith(".0.weight"):
            st[k] = (st[k] * g).astype(np.float32)
    for head in ("fc_block_4_mean", "fc_block_4_uncertainty"):
        k = f"model_last_block_list.0.{head}.1.weight"
        st[k] = (st[k] / g ** 7).astype(np.float32)
    return st


def overflow_pair():
    """the frame pair the repair test steps on (its sessions' last two frames) and the prior the search evaluates it with"""
    import test_gpu_filters as tg
    fr = tg._frames(np.random.default_rng(1), 12)
    return fr[10], fr[11], np.zeros(8)


def block4_activation_bound(oracle, img1, img2, prior):
    """per block-4 convolution, a lower bound of max |activation| in the oracle's prior-1 forward (the largest of the traced samples and |mean|),
    and the outputs"""
    r = oracle.forward(img1, img2, prior=prior, blocks_to_run=1, n_mc=ITER_MODEL["mc_samples"], p=ITER_MODEL["dropout_p"], mc_seed=9, pair_seq=1,
                       want_trace=True)
    lo = {n: max(float(np.abs(v[3:]).max()), abs(float(v[0])) / float(v[2])) for n, v in r["layer_stats"].items() if n.startswith("block_4_")}
    return lo, r


def overflow_checks(gain):
    """(largest weight, its bound, largest activation bound of block_4_0 .. 4_5, outputs finite)"""
    from cuahn_vio_amd import weights
    from oracle import pyoracle
    st = overflow_iterative_state(gain)
    rows, _mode = weights.weight_range_report(st)
    lo, r = block4_activation_bound(pyoracle.Oracle(weights.pack_state_dict(st)), *overflow_pair())
    act = max(v for n, v in lo.items() if n != "block_4_6")          # outputs that feed another convolution's fp16 planes
    return max(m for _n, m, _ok in rows), weights.F16X2_WEIGHT_BOUND, act, bool(np.isfinite(r["mean"]).all() and np.isfinite(r["cov"]).all())


def choose_overflow_gain():
    for g in OVERFLOW_GAINS:
        w, bound, act, finite = overflow_checks(g)
        if w < bound and act > FP16_MAX and finite:
            return g
    raise AssertionError("no gain of OVERFLOW_GAINS overflows the fp16 planes within the weight bound")


def overflow_iterative_blob():
    from cuahn_vio_amd import weights
    return weights.pack_state_dict(overflow_iterative_state(choose_overflow_gain()), variant=ITER_MODEL)


def test_iterative_symbols_are_exported_and_declared():
    _capi, L = _lib()
    header = open(os.path.join(ROOT, "include", "hnet.h")).read()
    for name in ("hnet_sessions_set_iterative_model", "hnet_sessions_infer_iter"):
        assert name in _capi.SYMBOLS and name in header
        getattr(L, name)


def test_iterative_calls_reject_null_sessions():
    _capi, L = _lib()
    ids = np.zeros(1, np.int32)
    mean, cov = np.zeros(8, np.float32), np.zeros(64, np.float32)
    assert L.hnet_sessions_set_iterative_model(None, None) == INVALID
    assert L.hnet_sessions_infer_iter(None, 1, 1, ids.ctypes.data, None, mean.ctypes.data, cov.ctypes.data, None) == INVALID
    assert L.hnet_sessions_infer_iter(None, 0, 1, ids.ctypes.data, None, mean.ctypes.data, cov.ctypes.data, None) == INVALID


class _NoCalls:
    """stands in for the library: any call into it fails the test"""
    calls = []

    def __getattr__(self, name):
        _NoCalls.calls.append(name)
        raise AssertionError(f"the wrapper called {name} before validating its arguments")


def _fake_sessions():
    from cuahn_vio_amd.homography_net import HnetSessions
    s = HnetSessions.__new__(HnetSessions)
    s._L, s._s, s.n, s.engine, s.iter_engine = _NoCalls(), ctypes.c_void_p(1), 4, None, None
    return s


def test_wrappers_validate_before_calling_the_library():
    _NoCalls.calls = []
    s = _fake_sessions()
    for bad in (-1, -5, 1.0, "1", True, None):
        with pytest.raises(ValueError):
            s.infer([0], prior=np.zeros((1, 8)), iteration=bad)
    for bad in ("engine", 12, object(), s):
        with pytest.raises(TypeError):
            s.set_iterative_model(bad)
    assert s.iter_engine is None
    assert _NoCalls.calls == []
    s._s = None                                                            # (nothing to destroy)


def test_overflow_weights_leave_the_fp16_range_in_activations_only():
    """the generator's properties on the CPU, with the oracle (the repair test's premises)"""
    g = choose_overflow_gain()
    w, bound, act, finite = overflow_checks(g)
    print(f"overflow gain {g}: max |w| = {w:.4f} (bound {bound}), block-4 activation >= {act:.4g} (fp16 max {FP16_MAX}), outputs finite: {finite}")
    assert w < bound and act > FP16_MAX and finite
    _w, _b, act_1, _f = overflow_checks(1.0)
    assert act_1 < 100.0                                                   # the unscaled weights stay far inside the range
