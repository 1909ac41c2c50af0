"""GPU: the heads' second FC, the uncertainty head's dropout streams and the ensemble (heads_fc2_chunk, heads_fc2_finish_kernel, heads_fc2_kernel,
mc_finish_kernel / mc_finish_wave, the gathered layout) with log-variances away from zero, against the double oracle and the reference model.

On every other weight set of the suite exp(logvar) is 1 to 4e-5 (tests/test_heads_range_cpu.py asserts it), so a finish that used 1.0 for it, read
another sample's or component's log-variance, or drew the uncertainty head's masks from the wrong stream would pass every older test.  Here the
log-variances span about [-5, 5] (weights.variant_state(unc_gain = 1e5)) or are drawn from [-8, 8].

Gates.  Means: conftest.tol_px_vs_oracle, unchanged.  Covariance: conftest.TOL_COV_REL as before AND, per entry of the 2 x 2 diagonal blocks,
|cov_ij - ref_ij| / sqrt(ref_ii ref_jj) < TOL_COV_ENTRY = 9.8e-6; per-sample log-variances: |logvar_s - oracle| < TOL_LOGVAR_S = 3.05e-5.
Both are 4 x the plain-fp32 oracle's error against the double oracle on the very pairs run here (2.45e-6; 7.63e-6), which is larger than the
reference's fp32 run against its fp64 run on tests/golden/heads_range (1.09e-6; 9.74e-7), and both stay below the cap of 2e-4: derivation and
figures in tests/heads_range.py, recomputed by test_heads_range_cpu.py::test_gate_basis.  The HIP path's own errors, per case and arithmetic mode,
are printed by every test and kept in profiles/heads_range_parity.csv (HNET_HEADS_RANGE_TABLE=<file> appends them)."""
import os

import numpy as np
import pytest

import heads_range as hr
from conftest import GOLDEN_DIR, TOL_COV_REL, TOL_PX_VS_ORACLE, TOL_PX_VS_REF32, TOL_PX_VS_REF64, tol_px_vs_oracle
from heads_range import MC_SEED, TOL_COV_ENTRY, TOL_LOGVAR_S
from test_gpu_parity import PRECISIONS

pytestmark = pytest.mark.gpu

MODE = {0: "fp32", 2: "bf16x3", 3: "f16x2"}


def _record(case, precision, mean_err, cov_rel, cov_entry, logvar_err=float("nan")):
    print(f"{case} [{MODE[precision]}]: |mean - ref| {mean_err:.2e} px, cov rel {cov_rel:.2e}, cov per entry {cov_entry:.2e}, logvar_s {logvar_err:.2e}")
    table = os.environ.get("HNET_HEADS_RANGE_TABLE")
    if table:
        new = not os.path.exists(table)
        with open(table, "a") as f:
            if new:
                f.write("case,precision,abs_err_mean_px,cov_rel_err,cov_entry_err,logvar_s_abs_err\n")
            f.write(f"{case},{MODE[precision]},{mean_err:.3e},{cov_rel:.3e},{cov_entry:.3e},{logvar_err:.3e}\n")


class _Engines:
    """the contexts of one arithmetic mode, created on first use and closed together"""

    def __init__(self, precision):
        self.precision, self._e = precision, {}

    def get(self, variant="full", n_mc=16, p=0.05, max_batch=12, mc_shard=None):
        from cuahn_vio_amd.homography_net import HnetEngine
        key = (variant, n_mc, p, max_batch, mc_shard)
        if key not in self._e:
            self._e[key] = HnetEngine(hr.weights_of()[1], variant=variant, mc_samples=n_mc, dropout_p=p, mc_seed=MC_SEED, max_batch=max_batch,
                                      mc_shard=mc_shard, precision=self.precision)
        return self._e[key]

    def close(self):
        for e in self._e.values():
            e.close()
        self._e = {}


@pytest.fixture(scope="module", params=PRECISIONS)
def engines(request):
    es = _Engines(request.param)
    yield es
    es.close()


def _errs(mean, cov, ref_mean, ref_cov):
    """(mean error in px, covariance error relative to max |ref|, per-entry covariance error) of one pair"""
    assert np.isfinite(mean).all() and np.isfinite(cov).all() and hr.outside_blocks_zero(cov)
    return (float(np.abs(mean - ref_mean).max()), float(np.abs(cov - ref_cov).max() / np.abs(ref_cov).max()), hr.cov_entry_err(cov, ref_cov))


def _gate(case, precision, errs):
    """records the worst pair's figures, then asserts every gate on every pair"""
    _record(case, precision, *np.max(np.array(errs), axis=0))
    for k, (dm, dr, de) in enumerate(errs):
        assert dm < tol_px_vs_oracle(precision), (case, k, dm)
        assert dr < TOL_COV_REL, (case, k, dr)
        assert de < TOL_COV_ENTRY, (case, k, de)


# ---- the forward on the wide variant, every finish path ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", hr.FORWARD_CASES, ids=[c["id"] for c in hr.FORWARD_CASES])
def test_forward_wide_variant_vs_oracle(engines, case):
    prev, curr, prior = hr.case_inputs(case)
    b = prev.shape[0]
    eng = engines.get(case["variant"], case["n_mc"], case["p"], max_batch=12 if b > 8 else 8)
    mean, cov = eng.infer_batch(prev, curr, prior, pair_seq0=case["seq0"])
    assert eng.precision() == engines.precision          # nothing overflowed: the context kept its arithmetic mode
    _gate(case["id"], engines.precision, [_errs(mean[k], cov[k], a["mean"], a["cov"]) for k, a in enumerate(hr.case_answers(case))])


def test_forward_sessions_with_unequal_sequence_numbers(engines):
    """HnetSessions.infer keys every pair with its session's own sequence number (the seq_tab form of the heads' kernels)"""
    from cuahn_vio_amd.homography_net import HnetSessions
    eng = engines.get("full", 16, 0.05, max_batch=8)
    s = HnetSessions(eng, len(hr.SESSION_SEEDS))
    ids = list(range(len(hr.SESSION_SEEDS)))
    try:
        for which in (0, 1):
            s.push(ids, np.stack([hr.pair(seed)[which] for seed in hr.SESSION_SEEDS]), [0.1 * which] * len(ids))
        for i, q in zip(ids, hr.SESSION_SEQS):
            s.set_seq(i, q)
        mean, cov = s.infer(ids)
    finally:
        s.close()
    assert eng.precision() == engines.precision
    refs = [hr.oracle_answer(seed, 16, 0.05, q) for seed, q in zip(hr.SESSION_SEEDS, hr.SESSION_SEQS)]
    _gate("sessions_b3_n16_full", engines.precision, [_errs(mean[k], cov[k], a["mean"], a["cov"]) for k, a in enumerate(refs)])


@pytest.mark.parametrize("name", hr.GOLDEN_NAMES)
def test_forward_wide_variant_vs_reference(engines, name):
    """batch 1 against the reference model's own fp32 and fp64 runs on the wide variant (tests/golden/heads_range)"""
    loaded = hr.load_golden(name)
    assert loaded is not None, "tests/golden/heads_range is part of the repository"
    g, i1, i2, prior, _btr = loaded
    n, p, seq = int(g["n_mc"]), float(g["p"]), int(g["pair_seq"])
    eng = engines.get(str(g["variant"]), n, p, max_batch=8)
    mean, cov = eng.infer_batch(i1[None], i2[None], None if prior is None else prior[None], pair_seq0=seq)
    assert np.isfinite(mean).all() and np.isfinite(cov).all() and eng.precision() == engines.precision
    d32, d64 = float(np.abs(mean[0] - g["mean"]).max()), float(np.abs(mean[0] - g["mean64"]).max())
    floor32 = float(np.abs(g["mean"] - g["mean64"]).max())
    e32, e64 = hr.cov_entry_err(cov[0], g["cov"]), hr.cov_entry_err(cov[0], g["cov64"])
    r64 = float(np.abs(cov[0] - g["cov64"]).max() / np.abs(g["cov64"]).max())
    _record(name.replace("heads_range/", "ref_"), engines.precision, d64, r64, max(e32, e64))
    assert d32 < max(TOL_PX_VS_REF32, floor32 + TOL_PX_VS_REF64) and d64 < TOL_PX_VS_REF64
    for ref in (g["cov"], g["cov64"]):
        assert np.abs(cov[0] - ref).max() / np.abs(ref).max() < TOL_COV_REL
    assert e32 < TOL_COV_ENTRY and e64 < TOL_COV_ENTRY
    assert hr.outside_blocks_zero(cov[0])


# ---- the per-sample outputs of a shard -------------------------------------------------------------------------------------------------------------
def test_shard_per_sample_outputs_vs_oracle(engines):
    """samples [5, 13) of N = 16 (s_begin != 0, not aligned to the chunk of four) of a 3-pair batch: heads_fc2_kernel's per-sample means and
    log-variances against Oracle.heads on the oracle's own traced features, H_part1 against the oracle's"""
    import torch
    from cuahn_vio_amd.homography_net import PIX_U8
    case = hr.FORWARD_CASES[0]
    s0, s1 = hr.SHARD
    prev, curr, _ = hr.case_inputs(case)
    b, nl = prev.shape[0], s1 - s0
    eng = engines.get("full", 16, 0.05, max_batch=8, mc_shard=hr.SHARD)
    dev = torch.device("cuda:0")
    tp, tc = torch.from_numpy(prev).to(dev), torch.from_numpy(curr).to(dev)
    ms, lv, h1 = torch.zeros(b, nl, 8, device=dev), torch.zeros(b, nl, 8, device=dev), torch.zeros(b, 9, device=dev)
    torch.cuda.synchronize()
    eng.infer_mc_partial_device(tp.data_ptr(), tc.data_ptr(), PIX_U8, None, b, case["seq0"], ms.data_ptr(), lv.data_ptr(), h1.data_ptr())
    assert eng.overflow_flag() == 0
    ms, lv, h1 = ms.cpu().numpy(), lv.cpu().numpy(), h1.cpu().numpy().reshape(b, 3, 3)
    errs = []
    for k, a in enumerate(hr.case_answers(case)):
        rm, rl = hr.oracle_of().heads(a["feat"], s0, s1, case["p"], MC_SEED, case["seq0"] + k)
        assert np.array_equal(rm, a["mean_s"][s0:s1]) and np.array_equal(rl, a["logvar_s"][s0:s1])
        assert rl.max() - rl.min() > 6.0
        errs.append((float(np.abs(ms[k] - rm).max()), float(np.abs(lv[k].astype(np.float64) - rl).max()), float(np.abs(h1[k] - a["H_part1"]).max())))
    worst = np.max(np.array(errs), axis=0)
    _record("shard_5_13_of_16_per_sample", engines.precision, worst[0], float("nan"), float("nan"), worst[1])
    for k, d in enumerate(errs):
        assert d[0] < tol_px_vs_oracle(engines.precision), (k, d)
        assert d[1] < TOL_LOGVAR_S, (k, d)
        assert d[2] < 2e-5, (k, d)


# ---- the finish operator alone -------------------------------------------------------------------------------------------------------------------
FINISH_B = 3
FINISH_N = [1, 2, 7, 8, 9, 33, 64, 65, 200]
GATHERED = {2: (2, 1), 9: (3, 3), 64: (4, 16), 200: (8, 25)}      # N -> world x n_local
# Kernel and oracle both carry the sums in double; what separates them is a handful of fp32 roundings of 6e-8 each (the fp32 mean, the two fp32
# variances, their sum, the stored value)
TOL_FINISH_COV_ENTRY = 1e-6
P4 = np.array([0, 0, 0, 223, 319, 223, 319, 0], np.float32)


def _finish_inputs(n):
    """(mean_s [B, N, 8], logvar_s [B, N, 8], H1 [B, 9]): means N(0, 5 px), log-variances uniform in [-8, 8] independently per sample and
    component, H1 the DLT of +-30 px corner offsets, the last pair's the `persp` homography of tests/golden/warp_s11.npz"""
    from oracle import pyoracle
    rng = np.random.default_rng(1000 + n)
    ms = (rng.standard_normal((FINISH_B, n, 8)) * 5.0).astype(np.float32)
    lv = rng.uniform(-8.0, 8.0, (FINISH_B, n, 8)).astype(np.float32)
    h1 = np.stack([pyoracle.dlt(P4 + rng.uniform(-30.0, 30.0, 8).astype(np.float32)).reshape(9) for _ in range(FINISH_B)]).astype(np.float32)
    h1[FINISH_B - 1] = np.load(os.path.join(GOLDEN_DIR, "warp_s11.npz"))["H_persp"].astype(np.float32).reshape(9)
    return ms, lv, h1


def _finish_all(eng, ms, lv, h1, gathered=None):
    """the entry points on the same samples -> {name: (mean [B, 8], cov [B, 8, 8])}, and the overflow word after them"""
    import torch
    dev = torch.device("cuda:0")
    b, n = ms.shape[:2]
    dms, dlv, dh = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (ms, lv, h1))
    mean, cov = torch.zeros(b, 8, device=dev), torch.zeros(b, 64, device=dev)
    o_packed, o_gath = torch.full((b, 72), -1.0, device=dev), torch.full((b, 72), -1.0, device=dev)
    torch.cuda.synchronize()
    eng.mc_finish_device(dms.data_ptr(), dlv.data_ptr(), n, dh.data_ptr(), b, mean.data_ptr(), cov.data_ptr())
    eng.mc_finish_packed_device(dms.data_ptr(), dlv.data_ptr(), n, dh.data_ptr(), b, o_packed.data_ptr())
    if gathered:
        world, nl = gathered
        assert world * nl == n
        # rank r's message: [mean block | log-variance block], each [B][n_local][8], of its samples [r * n_local, (r + 1) * n_local)
        buf = np.stack([np.stack([ms[:, r * nl:(r + 1) * nl], lv[:, r * nl:(r + 1) * nl]]) for r in range(world)])
        assert buf.shape == (world, 2, b, nl, 8)
        dg = torch.from_numpy(np.ascontiguousarray(buf)).to(dev)
        torch.cuda.synchronize()
        eng.mc_finish_gathered_device(dg.data_ptr(), world, nl, dh.data_ptr(), b, o_gath.data_ptr())
    flag = eng.overflow_flag()          # (synchronises)
    out = {"device": (mean.cpu().numpy(), cov.cpu().numpy().reshape(b, 8, 8))}
    for name, o in (("packed", o_packed),) + ((("gathered", o_gath),) if gathered else ()):
        o = o.cpu().numpy()
        out[name] = (o[:, :8].copy(), o[:, 8:].reshape(b, 8, 8).copy())
    return out, flag


@pytest.mark.parametrize("n", FINISH_N)
def test_finish_operator_vs_oracle(engines, n):
    ms, lv, h1 = _finish_inputs(n)
    out, flag = _finish_all(engines.get("full", 16, 0.05, max_batch=8), ms, lv, h1, GATHERED.get(n))
    assert flag == 0
    assert ("gathered" in out) == (n in GATHERED)
    mean, cov = out["device"]
    for name in out:           # the three entry points run one kernel on three layouts: the same bits
        assert np.array_equal(out[name][0], mean) and np.array_equal(out[name][1], cov), name
    errs = []
    for b in range(FINISH_B):
        rm, rc, _ = hr.oracle_of().finish(ms[b], lv[b], h1[b])
        errs.append(_errs(mean[b], cov[b], rm, rc))
    _record(f"finish_n{n}", engines.precision, *np.max(np.array(errs), axis=0))
    for b, (dm, _dr, de) in enumerate(errs):
        assert dm < TOL_PX_VS_ORACLE, (b, dm)
        assert de < TOL_FINISH_COV_ENTRY, (b, de)


@pytest.mark.parametrize("n", [1, 33])
def test_finish_log_variance_of_89(engines, n):
    """one log-variance of one pair at 89.0: exp of it (4.5e38) is beyond fp32.  At N = 1 it is that component's variance: the pair's entries are what
    Oracle.finish gives (+inf on the diagonal) and the overflow word reports bit 0.  At N = 33 the mean over the samples (1.4e37) still fits: finite,
    within the gate, no flag.  Either way every other value - the other pairs, this pair's means and other corners - keeps its bits."""
    pb, comp = 1, 3
    ms, lv, h1 = _finish_inputs(n)
    eng = engines.get("full", 16, 0.05, max_batch=8)
    clean, flag0 = _finish_all(eng, ms, lv, h1)
    bad_lv = lv.copy()
    bad_lv[pb, min(7, n - 1), comp] = 89.0
    overflows = bool(np.exp(89.0) / n > np.finfo(np.float32).max)
    assert overflows == (n == 1)
    got, flag1 = _finish_all(eng, ms, bad_lv, h1)
    assert flag0 == 0 and (flag1 & 1) == int(overflows)
    assert eng.overflow_flag() == 0                          # reading the word cleared it
    with np.errstate(all="ignore"):
        _rm, rc, _ = hr.oracle_of().finish(ms[pb], bad_lv[pb], h1[pb])
    fin = np.isfinite(rc)
    assert fin.all() != overflows
    corner = np.zeros((8, 8), bool)
    corner[2 * (comp // 2):2 * (comp // 2) + 2, 2 * (comp // 2):2 * (comp // 2) + 2] = True
    for name in ("device", "packed"):
        mean, cov = got[name]
        assert np.array_equal(mean, clean[name][0])          # the means do not depend on the log-variances
        assert np.array_equal(np.isfinite(cov[pb]), fin) and np.array_equal(cov[pb][~fin], rc[~fin], equal_nan=True)
        if overflows:
            assert rc[comp, comp] == np.inf and cov[pb][comp, comp] == np.inf
        else:
            assert cov[pb][comp, comp] > 1e36 and hr.cov_entry_err(cov[pb], rc) < TOL_FINISH_COV_ENTRY
        assert np.array_equal(cov[pb][~corner], clean[name][1][pb][~corner])
        for b in range(FINISH_B):
            if b != pb:
                assert np.array_equal(cov[b], clean[name][1][b])


def test_host_call_on_weights_whose_variance_overflows():
    """unc_gain = 3e6: the oracle's ensemble variance of four components is beyond fp32 (ln of it 100 ... 127), so the covariance holds +-inf where
    the reference model's would.  A host-result call in the default arithmetic takes the non-finite output for an fp16-plane overflow, demotes the
    context to split-bf16 once and runs again (run_host_call): the call returns OK, the means are the oracle's, the non-finite entries are where
    and what the oracle has, and the result is reproducible.  Such a file ends in HNET_PREC_BF16X3 (parity section)."""
    from cuahn_vio_amd.homography_net import HnetEngine
    gain, seeds, seq0 = 3e6, (12, 13), 7
    refs = [hr.oracle_answer(s, 16, 0.05, seq0 + k, unc_gain=gain) for k, s in enumerate(seeds)]
    for a in refs:
        assert np.isfinite(a["mean"]).all() and 0 < (~np.isfinite(a["cov"])).sum() < 16 and not np.isnan(a["cov"]).any()
    prev, curr = np.stack([hr.pair(s)[0] for s in seeds]), np.stack([hr.pair(s)[1] for s in seeds])
    eng = HnetEngine(hr.weights_of(gain)[1], variant="full", mc_samples=16, dropout_p=0.05, mc_seed=MC_SEED, max_batch=2, precision=3)
    try:
        assert eng.precision() == 3
        mean, cov = eng.infer_batch(prev, curr, pair_seq0=seq0)          # returns OK (an error status raises)
        assert eng.precision() == 2
        mean2, cov2 = eng.infer_batch(prev, curr, pair_seq0=seq0)
        assert eng.precision() == 2
    finally:
        eng.close()
    assert np.array_equal(mean, mean2) and np.array_equal(cov, cov2, equal_nan=True)
    for k, a in enumerate(refs):
        assert np.isfinite(mean[k]).all() and np.abs(mean[k] - a["mean"]).max() < tol_px_vs_oracle(2)
        fin = np.isfinite(a["cov"])
        assert np.array_equal(np.isfinite(cov[k]), fin), k
        assert np.array_equal(cov[k][~fin], a["cov"][~fin], equal_nan=True), k
        assert hr.outside_blocks_zero(cov[k])
