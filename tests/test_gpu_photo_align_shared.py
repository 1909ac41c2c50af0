"""The three photometric alignment calls side by side on one context (include/hnet.h hnet_op_photo_align, hnet_op_photo_align_pyramid,
hnet_op_photo_align_robust): they share their level driver, the front of their solve kernels and the context's scratch, so a record must
not depend on which of them ran before.  Every record of every level of interleaved calls equals, byte for byte, that of a context which makes one kind of call only;
and with the model off the robust call's px part is the pyramid call's at every number of levels at n = 1."""
import numpy as np
import pytest

import photo_align_util as U
import photo_hostile as H

pytestmark = pytest.mark.gpu

K = 3
KINDS = ("plain", "pyramid", "robust")
BATCHES = ((0, 1, 2), (0,), (1,), (2,))          # n = 3, and every pair alone
ORDINARY, OUTSIDE, DEGENERATE = 0, 1, 2          # the pairs of the batch


@pytest.fixture(scope="module")
def data():
    """an ordinary pair from 0.75 px, a pair whose start puts every pixel outside img2, a pair whose start has its four corners on a line"""
    s = U.smooth_pair(5, 8.0)
    i1, i2 = np.stack([s[0]] * 3), np.stack([s[1]] * 3)
    return i1, i2, np.stack([np.full(8, 0.75, np.float32), H.cand("far"), H.cand("line")])


def _engine(blob):
    from cuahn_vio_amd.homography_net import HnetEngine
    return HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=3)


def _call(e, kind, data, idx):
    """one call on the pairs idx -> (the bytes of out and of levels_out, the flags [n, levels])"""
    i1, i2, start = (np.ascontiguousarray(x[list(idx)]) for x in data)
    if kind == "plain":
        out = e.op_photo_align(i1, i2, start, max_iterations=K)
        return out.tobytes(), out["flags"][:, None]
    if kind == "pyramid":
        out, lv = e.op_photo_align_pyramid(i1, i2, start, levels=4, want_levels=True, max_iterations=K)
        return out.tobytes() + lv.tobytes(), lv["flags"]
    out, lv = e.op_photo_align_robust(i1, i2, start, levels=4, want_levels=True, max_iterations=K, brightness=1, huber_k=10.0)
    return out.tobytes() + lv.tobytes(), lv["px"]["flags"]


@pytest.fixture(scope="module")
def twins(blob, data):
    """{(kind, idx): bytes} from three contexts each of which makes one kind of call only; the stopped pairs stop as they are meant to at every level"""
    want = {}
    for kind in KINDS:
        e = _engine(blob)
        for idx in BATCHES:
            want[kind, idx], flags = _call(e, kind, data, idx)
            for b, p in enumerate(idx):
                if p == OUTSIDE:
                    assert (flags[b] & H.FEW_PIXELS).all(), (kind, idx, flags[b])
                elif p == DEGENERATE:
                    assert (flags[b] & H.DEGENERATE).all(), (kind, idx, flags[b])
                else:
                    assert not (flags[b] & (H.FEW_PIXELS | H.DEGENERATE | H.SINGULAR)).any(), (kind, idx, flags[b])
        e.close()
    return want


@pytest.mark.parametrize("order", [("plain", "pyramid", "robust"), ("robust", "pyramid", "plain")], ids=lambda o: "-".join(o))
def test_interleaved_calls_equal_single_kind_contexts(blob, data, twins, order):
    """one context, the three calls in `order`, batch after batch (n = 3, then each pair alone), twice over: every record of every level is the twin's"""
    e = _engine(blob)
    try:
        for rnd in range(2):
            for idx in BATCHES:
                for kind in order:
                    got, _ = _call(e, kind, data, idx)
                    assert got == twins[kind, idx], (rnd, idx, kind)
    finally:
        e.close()


def test_model_off_is_the_pyramid_call_at_one_pair(blob, data):
    """brightness = 0 and huber_k = 0 at n = 1, levels 1 - 4, for each of the three pairs: the px part of every record equals the pyramid call's bytes"""
    e = _engine(blob)
    try:
        for p in range(3):
            i1, i2, start = (np.ascontiguousarray(x[p:p + 1]) for x in data)
            for levels in (1, 2, 3, 4):
                want, wlv = e.op_photo_align_pyramid(i1, i2, start, levels=levels, want_levels=True, max_iterations=K)
                out, lv = e.op_photo_align_robust(i1, i2, start, levels=levels, want_levels=True, max_iterations=K, brightness=0, huber_k=0.0)
                assert np.ascontiguousarray(out["px"]).tobytes() == want.tobytes(), (p, levels)
                assert np.ascontiguousarray(lv["px"]).tobytes() == wlv.tobytes(), (p, levels)
    finally:
        e.close()
