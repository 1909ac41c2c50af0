"""Photometric alignment on the device (include/hnet.h hnet_photo_align; csrc/kernels_photo_align.hip): the operator call against the host
reference tests/cpp/photo_align_ref.cpp and the truth of synthetic pairs, shapes and bitwise independence of the batch, the degenerate inputs, the
read-only sessions call and the consistency with the residual records.  Main model prior-3, N = 16, max_batch 9."""
import ctypes as C

import numpy as np
import pytest

import photo_align_util as U

pytestmark = pytest.mark.gpu

INVALID, NOT_READY, CAPACITY = 1, 4, 5
# Measured on an MI355X (printed by the tests below), each gated at 10 x the measurement:
#   K = 0, device against host reference, worst relative difference over the 3 pairs (summation order only: every product of two floats is exact in a double)
MEASURED_LIN = {"mse": 1.3e-13, "grad": 2.6e-13, "info": 5.9e-13}
#   K = 6 and K = 10, worst |device offsets - reference offsets| over the 12 pairs, px: measured 0 (every trial, decision and final offset equal); the gate
#   is never set below the granularity of the fp32 offsets themselves (one ulp of an offset between 8 and 16 px, 9.5e-7 px)
MEASURED_OFFSETS_PX = 0.0
OFFSET_ULP_PX = 2.0 ** -20


@pytest.fixture(scope="module")
def aref(tmp_path_factory):
    return U.build_ref(tmp_path_factory.mktemp("photo_align_ref_gpu"))


@pytest.fixture(scope="module")
def eng(blob):
    from cuahn_vio_amd.homography_net import HnetEngine
    e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=9)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cases():
    c = U.convergence_cases()
    return {"names": [x[0] for x in c], "i1": np.stack([x[1] for x in c]), "i2": np.stack([x[2] for x in c]), "truth": np.stack([x[3] for x in c]),
            "start": np.stack([x[4] for x in c]), "gate": np.array([x[5] for x in c])}


@pytest.fixture(scope="module")
def ref_runs(aref, cases):
    """the host reference on the 12 convergence pairs at K = 6 and K = 10, once for the module"""
    return {K: U.ref_run(aref, cases["i1"], cases["i2"], cases["start"], max_iterations=K) for K in (6, 10)}


@pytest.fixture(scope="module")
def dev_runs(eng, cases):
    """the device on the same pairs (9 + 3: max_batch is 9), once for the module"""
    out = {}
    for K in (6, 10):
        parts = [eng.op_photo_align(cases["i1"][a:b], cases["i2"][a:b], cases["start"][a:b], max_iterations=K) for a, b in ((0, 9), (9, 12))]
        out[K] = np.concatenate(parts)
    return out


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / np.sqrt((b ** 2).sum()))


def test_linearisation_matches_reference(eng, aref):
    """a. K = 0 on two smooth pairs and one stock pair: n_valid equal; mse, grad and info (Frobenius) differ from the host reference by summation order
    alone.  Measured worst relative difference: see MEASURED_LIN; gated at 10 x that, and never accepted above 1e-6 (something other than rounding)."""
    s1, s2, st = U.smooth_pair(1, 2.0), U.smooth_pair(5, 8.0), U.stock_pair(2)
    i1, i2 = np.stack([s1[0], s2[0], st[0]]), np.stack([s1[1], s2[1], st[1]])
    start = np.stack([np.zeros(8, np.float32), np.full(8, 0.75, np.float32), st[3]])
    dev = eng.op_photo_align(i1, i2, start, max_iterations=0)
    ref = U.ref_run(aref, i1, i2, start, max_iterations=0)
    worst = {"mse": 0.0, "grad": 0.0, "info": 0.0}
    for b in range(3):
        assert dev["n_valid"][b] == ref["n_valid"][b] == dev["n_valid0"][b] and dev["flags"][b] == ref["flags"][b] == 0
        assert dev["trials"][b] == 0 and dev["offsets_px"][b].tobytes() == start[b].tobytes() and dev["mse"][b] == dev["mse0"][b]
        assert (dev["info"][b] == dev["info"][b].T).all()
        worst["mse"] = max(worst["mse"], abs(dev["mse"][b] - ref["mse"][b]) / ref["mse"][b])
        worst["grad"] = max(worst["grad"], _rel(dev["grad"][b], ref["grad"][b]))
        worst["info"] = max(worst["info"], _rel(dev["info"][b], ref["info"][b]))
    print("K = 0, device vs host reference, worst relative difference:", {k: f"{v:.3e}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= 1e-6, k
        assert v <= 10 * MEASURED_LIN[k], k


@pytest.mark.parametrize("K", [6, 10])
def test_alignment_matches_reference_and_truth(cases, ref_runs, dev_runs, K):
    """b. the pairs of the CPU convergence test (seeds 1, 2, 5, 11; smooth at max_offset 2 and 8 from zero, stock from the sigma = 1 prior): flags,
    trials and accepted counts equal the host reference's; the final offsets lie within 10 x MEASURED_OFFSETS_PX of it; and, at K = 6 as at K = 10,
    within 0.05 px (smooth) / 0.1 px (stock) of the true offsets in every component (measured at either K: smooth <= 0.019 px, stock <= 0.039 px)."""
    dev, ref = dev_runs[K], ref_runs[K]
    worst = 0.0
    for i, name in enumerate(cases["names"]):
        d, r = dev[i], ref[i]
        err = float(np.abs(d["offsets_px"].astype(np.float64) - cases["truth"][i]).max())
        diff = float(np.abs(d["offsets_px"].astype(np.float64) - r["offsets_px"]).max())
        worst = max(worst, diff)
        print(f"{name} K={K}: {err:.4f} px from the truth, {diff:.2e} px from the reference; flags {d['flags']}, trials {d['trials']}, accepted {d['accepted']}, "
              f"mse {d['mse0']:.3f} -> {d['mse']:.3f}")
        assert (d["flags"], d["trials"], d["accepted"]) == (r["flags"], r["trials"], r["accepted"]), name
        assert d["mse"] <= d["mse0"] and d["accepted"] <= d["trials"] <= K
        assert d["n_valid"] == r["n_valid"] and d["n_valid0"] == r["n_valid0"], name
        assert err < cases["gate"][i], name
    print(f"K = {K}: worst |device - reference| offsets {worst:.3e} px")
    assert worst <= max(10 * MEASURED_OFFSETS_PX, OFFSET_ULP_PX)


def test_shapes_and_batch_independence(eng, cases, dev_runs):
    """c. n = 1, 3, 8 and n = 9 at max_batch 9: a pair's whole record is bitwise the same alone, in slot 0, in the last slot and across two runs; a pair
    that converges after 4 trials keeps its bits beside one that uses all 10; and the refusals, which leave `out` untouched"""
    from cuahn_vio_amd import _capi
    i1, i2, start = cases["i1"], cases["i2"], cases["start"]
    nine = dev_runs[10][:9]
    alone = [eng.op_photo_align(i1[i], i2[i], start[i], max_iterations=10) for i in (0, 1, 2, 8)]            # n = 1
    for k, i in enumerate((0, 1, 2, 8)):
        assert alone[k][0].tobytes() == nine[i].tobytes(), i                                                   # alone == slot i of n = 9 (8: the last slot)
    three = eng.op_photo_align(i1[[8, 4, 0]], i2[[8, 4, 0]], start[[8, 4, 0]], max_iterations=10)               # n = 3: pair 0 last, pair 8 in slot 0
    assert three[0].tobytes() == nine[8].tobytes() and three[1].tobytes() == nine[4].tobytes() and three[2].tobytes() == nine[0].tobytes()
    order = [7, 1, 2, 3, 4, 5, 6, 0]
    eight = eng.op_photo_align(i1[order], i2[order], start[order], max_iterations=10)                           # n = 8
    for k, i in enumerate(order):
        assert eight[k].tobytes() == nine[i].tobytes(), i
    assert eng.op_photo_align(i1[order], i2[order], start[order], max_iterations=10).tobytes() == eight.tobytes()      # a second run
    quick, slow = cases["names"].index("smooth8-11"), cases["names"].index("stock-1")
    both = dev_runs[10][[quick, slow]]
    assert both["flags"][0] == U.CONVERGED and both["trials"][0] < 10 and both["flags"][1] == 0 and both["trials"][1] == 10
    pair = eng.op_photo_align(i1[[quick, slow]], i2[[quick, slow]], start[[quick, slow]], max_iterations=10)
    assert pair.tobytes() == both.tobytes()
    # refusals write nothing
    L = _capi.lib()
    out = np.full(10 * _capi.PHOTO_ALIGN_DTYPE.itemsize, 0xA5, np.uint8)
    keep = out.copy()
    a, b = np.ascontiguousarray(np.concatenate([i1[:9], i1[:1]])), np.ascontiguousarray(np.concatenate([i2[:9], i2[:1]]))
    x0 = np.zeros((10, 8), np.float32)
    ok = _capi.photo_align_opts()

    def call(n, o, img1=a.ctypes.data, outp=out.ctypes.data):
        return L.hnet_op_photo_align(eng.handle, img1, b.ctypes.data, n, x0.ctypes.data, C.addressof(o) if o is not None else None, outp)
    assert call(10, ok) == CAPACITY
    assert call(1, _capi.photo_align_opts(max_iterations=33)) == INVALID and call(1, _capi.photo_align_opts(min_valid=-1)) == INVALID
    assert call(1, _capi.photo_align_opts(lambda0=1.0000001e100)) == INVALID                                    # (lambda0 is capped: lambda cannot overflow)
    assert call(1, ok, img1=None) == INVALID and call(1, None) == INVALID and call(1, ok, outp=None) == INVALID and call(0, ok) == INVALID
    assert out.tobytes() == keep.tobytes()
    assert call(1, _capi.photo_align_opts(max_iterations=32)) == 0 and out.tobytes() != keep.tobytes()          # (the largest K is legal)


def test_degenerate_inputs_on_device(eng, aref):
    """d. the degenerate inputs of the CPU test in one call, at K = 6 and K = 0: the reference's flags, and its bits where they are exact (a zero
    information matrix, the start offsets); nothing non-finite"""
    cs = U.degenerate_cases()
    i1, i2, start = np.stack([c[1] for c in cs]), np.stack([c[2] for c in cs]), np.stack([c[3] for c in cs])
    for K in (6, 0):
        dev = eng.op_photo_align(i1, i2, start, max_iterations=K)
        ref = U.ref_run(aref, i1, i2, start, max_iterations=K)
        for b, (name, _a, _b, _s, flag, zero) in enumerate(cs):
            d = dev[b]
            assert d["flags"] == flag == ref["flags"][b], name
            assert d["offsets_px"].tobytes() == start[b].tobytes() and d["trials"] == 0 and d["accepted"] == 0
            assert d["n_valid0"] == ref["n_valid0"][b] and d["n_valid"] == ref["n_valid"][b]
            for f in ("mse0", "mse", "lambda", "grad", "info"):
                assert np.isfinite(d[f]).all(), (name, f)
            if zero:
                assert not d["info"].any() and not d["grad"].any()
            else:
                assert _rel(d["info"], ref["info"][b]) < 1e-6
            if flag in (U.DEGENERATE, U.FEW_PIXELS):
                assert d["mse0"] == 0.0 and d["mse"] == 0.0 and d["n_valid0"] == 0


def test_sessions_call_is_read_only(blob, eng):
    """e. hnet_sessions_photo_align on 3 sessions equals the operator call on hnet_sessions_get_frame's frames, bitwise; image counts, sequence numbers,
    times and last_timing are unchanged, and the next hnet_sessions_infer is bit-identical to that of a twin that never aligned; a one-image session and
    a repeated id are refused"""
    from cuahn_vio_amd import _capi
    from cuahn_vio_amd.homography_net import HnetEngine, HnetSessions
    pairs = [U.smooth_pair(1, 2.0), U.smooth_pair(2, 8.0), U.stock_pair(5)[:3], U.smooth_pair(11, 2.0)]

    def make():
        e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=9)
        s = HnetSessions(e, 5)
        for k in (0, 1):
            s.push([0, 1, 2, 3], np.stack([p[k] for p in pairs]), t=[1.0 + k] * 4)
        s.push([4], pairs[0][0][None], t=[1.0])
        s.set_seq(2, 41)
        s.infer([2, 0], np.zeros((2, 8)))                                    # (so that last_timing holds something)
        return e, s
    (e1, s1), (e2, s2) = make(), make()
    ids = np.array([3, 0, 2], np.int32)
    start = np.stack([np.zeros(8, np.float32), np.zeros(8, np.float32), U.stock_pair(5)[3]])
    state = lambda s: ([s.image_count(i) for i in range(5)], [s.seq(i) for i in range(5)], [s.latest_time(i) for i in range(5)], s.last_timing())
    before = state(s1)
    rec = s1.photo_align(ids, start, max_iterations=6)
    assert state(s1) == before
    prev, curr = np.stack([s1.frame(int(i), 0) for i in ids]), np.stack([s1.frame(int(i), 1) for i in ids])
    assert (prev[1] == pairs[0][0]).all() and (curr[1] == pairs[0][1]).all()
    assert rec.tobytes() == eng.op_photo_align(prev, curr, start, max_iterations=6).tobytes()
    assert rec["accepted"].min() >= 1 and e1.last_photo_align_device_ms() > 0.0
    prior = np.array(rec["offsets_px"], np.float64)
    m1, c1 = s1.infer(ids, prior)
    m2, c2 = s2.infer(ids, prior)
    assert m1.tobytes() == m2.tobytes() and c1.tobytes() == c2.tobytes() and state(s1)[:3] == state(s2)[:3]
    for bad, status in (([3, 4], NOT_READY), ([3, 3], INVALID), ([5], INVALID), (list(range(5)) * 2, CAPACITY)):
        with pytest.raises(_capi.HnetError) as ei:
            s1.photo_align(bad, np.zeros((len(bad), 8), np.float32))
        assert ei.value.status == status, bad
    with pytest.raises(_capi.HnetError) as ei:
        s1.photo_align(ids, start, max_iterations=33)
    assert ei.value.status == INVALID
    for o in (s1, e1, s2, e2):
        o.close()


def test_consistent_with_residual_records(eng):
    """f. mse and the residual record describe the same map.  On the identity hypothesis n_valid = 223 * 319 and n_inside = 71 680, the valid pixels are
    columns 0 - 318 of rows 0 - 222, and mse * n_valid is the float64 sum of the squared map over that block (|r| has the map's bits; what is left is the
    order of 71 137 additions, 1e-12); by Cauchy-Schwarz sqrt(mse) is at least the block's mean |e|.  At any hypothesis the valid pixels are a subset of
    all pixels: mse * n_valid <= the sum of the squared map."""
    i1, i2, off = U.stock_pair(1)[:3]
    offs = np.stack([np.zeros(8, np.float32), off.astype(np.float32)])
    rec, emap = eng.op_photo_residual(np.stack([i1, i1]), np.stack([i2, i2]), offs[:, None, :], want_map=True)
    al = eng.op_photo_align(np.stack([i1, i1]), np.stack([i2, i2]), offs, max_iterations=0)
    assert al["n_valid"][0] == 223 * 319 and rec["n_inside"][0, 0] == 71680
    block = emap[0, 0, :223, :319].astype(np.float64)
    want = float((block ** 2).sum())
    got = al["mse"][0] * al["n_valid"][0]
    print(f"identity: mse * n_valid {got:.6f} vs the map's {want:.6f} ({abs(got - want) / want:.1e}); rms {np.sqrt(al['mse'][0]):.4f}, "
          f"mean |e| inside {rec['sum_inside'][0, 0] / rec['n_inside'][0, 0]:.4f}")
    assert abs(got - want) <= 1e-12 * want
    assert np.sqrt(al["mse"][0]) >= block.mean() * (1 - 1e-12)
    assert 60000 < al["n_valid"][1] <= rec["n_inside"][1, 0]
    assert al["mse"][1] * al["n_valid"][1] <= float((emap[1, 0].astype(np.float64) ** 2).sum()) * (1 + 1e-12)
    assert al["mse"][1] < 0.5 * al["mse"][0]                                 # (the truth explains the pair better than no motion)
