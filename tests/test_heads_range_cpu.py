"""CPU: the uncertainty head and the ensemble away from the identity.

Every other weight set of the suite leaves fc_block_4_uncertainty at PyTorch's default initialisation: its per-sample log-variances are
+-4e-5, exp of them is 1 to 4e-5, and the only covariance gate (conftest.TOL_COV_REL = 2e-5 of max |cov|) cannot tell exp(logvar) from 1.0,
one sample's or component's log-variance from another's, or the uncertainty head's dropout streams from any other.  weights.variant_state
(unc_gain = 1e5) spreads the log-variances over about [-5, 5].  Here: the keyword leaves every existing blob byte-identical; the premise, as
assertions on the double oracle; and the oracle (double and plain fp32) against the reference model's own outputs on that variant
(tests/golden/heads_range, tools/gen_golden.py --group heads_range), per-sample head outputs included."""
import hashlib

import numpy as np
import pytest

import heads_range as hr
from conftest import TOL_COV_REL
from heads_range import TOL_COV_ENTRY, TOL_LOGVAR_S, UNC_GAIN

LB = "model_last_block_list.0.fc_block_4_uncertainty.4"

# sha256 of pack_state_dict(variant_state(seed, conv_gain)) before the keyword existed
PARENT_BLOBS = {(0, 1.0): "94a26edd0e544c2a2ef8b475fff048cfc03d05c5eeb43c62919e844bb9e88fbc",
                (1, 1.0): "1d462dc3f7e25082f0a3057230390581f4c80229611ef809e85420c9a26c71ee",
                (2, 4.0): "76458393915941d1b1dc6b65bd952efec5704dfb7eef1f574d153058930d6dcc",
                (3, 0.5): "a4d190459408aa3078a506cb7f88076310446f89fef3414b61fa3987db9c46f9"}


@pytest.mark.parametrize("key", sorted(PARENT_BLOBS))
def test_default_unc_gain_leaves_the_blob_byte_identical(key):
    from cuahn_vio_amd import weights
    b = weights.pack_state_dict(weights.variant_state(*key))
    assert hashlib.sha256(b).hexdigest() == PARENT_BLOBS[key]
    assert weights.pack_state_dict(weights.variant_state(*key, unc_gain=1.0)) == b
    if key == (0, 1.0):
        assert weights.pack_state_dict(weights.synthetic_state(0)) == b


def test_unc_gain_scales_the_last_layer_of_the_uncertainty_head_only():
    from cuahn_vio_amd import weights
    base, wide = weights.variant_state(2, 4.0), weights.variant_state(2, 4.0, unc_gain=UNC_GAIN)
    assert list(base) == list(wide)
    for k in base:
        if k in (LB + ".weight", LB + ".bias"):
            assert np.array_equal(wide[k], (base[k] * np.float32(UNC_GAIN)).astype(np.float32)) and wide[k].dtype == np.float32
            assert np.abs(wide[k]).max() > 1e3
        else:
            assert np.array_equal(base[k], wide[k]), k


# ---- the premise ------------------------------------------------------------------------------------------------------------------------------
def _terms(a):
    """(epistemic, aleatoric) [8] of an oracle answer: mean_i (m_bar - m_i)^2 and mean_i exp(logvar_i)  (model_to_trace.py:274-280)"""
    ms, lv = a["mean_s"].astype(np.float64), a["logvar_s"].astype(np.float64)
    return ((ms.mean(0) - ms) ** 2).mean(0), np.exp(lv).mean(0)


@pytest.mark.parametrize("seed", [12, 13])
def test_committed_weights_keep_the_log_variances_at_zero(seed):
    """why the cases on synthetic_state / variant_state(seed, conv_gain) cannot see this code: |logvar| < 1e-4 on every sample and component"""
    for p in (0.05, 0.5):
        a = hr.oracle_answer(seed, 16, p, seed, unc_gain=1.0)
        assert np.abs(a["logvar_s"]).max() < 1e-4
        assert np.isfinite(a["mean"]).all() and np.isfinite(a["cov"]).all()
        assert np.abs(np.exp(a["logvar_s"].astype(np.float64)) - 1.0).max() < 1e-4


@pytest.mark.parametrize("seed", [12, 13])
def test_wide_variant_spans_a_real_range(seed):
    for n, p in ((16, 0.05), (5, 0.5), (16, 0.5)):
        a = hr.oracle_answer(seed, n, p, seed)
        for v in a.values():
            assert np.isfinite(v).all()
        lv, d = a["logvar_s"], np.diag(a["cov"]).astype(np.float64)
        assert lv.max() - lv.min() >= 6.0
        assert d.min() > 0 and d.max() / d.min() >= 100.0
        epi, ale = _terms(a)
        if p == 0.5:       # heavy dropout: the spread of the means is of the order of the smallest aleatoric term
            assert (epi / (epi + ale)).max() >= 0.10
        # the per-sample log-variances differ from sample to sample and from component to component by far more than any gate
        assert np.abs(lv - lv[::-1]).max() > 0.1 and np.abs(lv - lv[:, ::-1]).max() > 1.0


def test_oracle_forward_is_heads_and_finish_on_its_traced_trunk():
    """heads_range.oracle_answer assembles the oracle's forward from one traced trunk: the same bits as Oracle.forward"""
    case = hr.FORWARD_CASES[2]
    i1, i2 = hr.pair(case["seeds"][0])
    pr = hr.prior_of(case["seeds"][0], case["prior_amp"])
    for f32 in (False, True):
        o = hr.oracle_of(f32=f32).forward(i1, i2, pr, 3, case["n_mc"], case["p"], hr.MC_SEED, case["seq0"])
        a = hr.case_answers(case, f32)[0]
        assert np.array_equal(o["mean"], a["mean"]) and np.array_equal(o["cov"], a["cov"])
    i1, i2 = hr.pair(13)
    o = hr.oracle_of().forward(i1, i2, None, 3, 5, 0.5, hr.MC_SEED, 51)
    a = hr.case_answers(hr.FORWARD_CASES[1])[1]
    assert np.array_equal(o["mean"], a["mean"]) and np.array_equal(o["cov"], a["cov"])


def test_gate_basis():
    """the figures TOL_COV_ENTRY and TOL_LOGVAR_S are 4 x of: the plain-fp32 oracle against the double oracle on every pair the GPU file runs, and
    the reference's fp32 run against its fp64 run on the committed files"""
    cov_o = lv_o = cov_r = lv_r = 0.0
    cases = hr.FORWARD_CASES + [dict(id="sessions", n_mc=16, p=0.05, seeds=hr.SESSION_SEEDS)]
    for case in cases:
        for k, s in enumerate(case["seeds"]):
            seq = hr.SESSION_SEQS[k] if case["id"] == "sessions" else case["seq0"] + k
            a = hr.oracle_answer(s, case["n_mc"], case["p"], seq, case.get("prior_amp"))
            b = hr.oracle_answer(s, case["n_mc"], case["p"], seq, case.get("prior_amp"), f32=True)
            cov_o = max(cov_o, hr.cov_entry_err(b["cov"], a["cov"]))
            lv_o = max(lv_o, float(np.abs(b["logvar_s"].astype(np.float64) - a["logvar_s"]).max()))
    for name in hr.GOLDEN_NAMES:
        g = hr.load_golden(name)[0]
        cov_r = max(cov_r, hr.cov_entry_err(g["cov"], g["cov64"]))
        lv_r = max(lv_r, float(np.abs(g["logvar_s32"] - g["logvar_s"]).max()))
    print(f"cov per entry: oracle f32 vs f64 {cov_o:.3e}, reference fp32 vs fp64 {cov_r:.3e}; logvar_s: oracle {lv_o:.3e}, reference {lv_r:.3e}")
    assert max(cov_o, cov_r) <= hr.MEASURED_COV_ENTRY * 1.02 and max(lv_o, lv_r) <= hr.MEASURED_LOGVAR_S * 1.02
    assert TOL_COV_ENTRY <= 2e-4 and TOL_LOGVAR_S <= 2e-4
    assert TOL_COV_ENTRY == pytest.approx(4 * hr.MEASURED_COV_ENTRY) and TOL_LOGVAR_S == pytest.approx(4 * hr.MEASURED_LOGVAR_S)


# ---- the oracle against the reference model on the wide variant ----------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [pytest.param(False, id="double"), pytest.param(True, id="f32")])
@pytest.mark.parametrize("name", hr.GOLDEN_NAMES)
def test_oracle_matches_reference_on_the_wide_variant(name, f32):
    loaded = hr.load_golden(name)
    assert loaded is not None, "tests/golden/heads_range is part of the repository (tools/gen_golden.py --group heads_range)"
    g, i1, i2, prior, btr = loaded
    assert float(g["unc_gain"]) == UNC_GAIN and int(g["weights_seed"]) == 0 and float(g["conv_gain"]) == 1.0 and int(g["mc_seed"]) == hr.MC_SEED
    n, p, seq = int(g["n_mc"]), float(g["p"]), int(g["pair_seq"])
    assert g["logvar_s"].shape == (n, 8) and g["logvar_s"].max() - g["logvar_s"].min() >= 6.0      # the reference itself spans the range
    orc = hr.oracle_of(f32=f32)
    o = orc.forward(i1, i2, prior, btr, n, p, hr.MC_SEED, seq, want_trace=True)
    d64, d32 = float(np.abs(o["mean"] - g["mean64"]).max()), float(np.abs(o["mean"] - g["mean"]).max())
    e64, e32 = hr.cov_entry_err(o["cov"], g["cov64"]), hr.cov_entry_err(o["cov"], g["cov"])
    ms, lv = orc.heads(o["feat"], 0, n, p, hr.MC_SEED, seq)
    dms, dlv = float(np.abs(ms - g["mean_s"]).max()), float(np.abs(lv - g["logvar_s"]).max())
    print(f"{name} [{'f32' if f32 else 'double'}]: mean {d64:.2e} / {d32:.2e} px vs ref fp64 / fp32, cov per entry {e64:.2e} / {e32:.2e}, "
          f"mean_s {dms:.2e} px, logvar_s {dlv:.2e}")
    if f32:      # the gates of test_oracle_f32_build_matches_reference
        assert d32 < 4e-4
        assert np.abs(o["cov"] - g["cov"]).max() / np.abs(g["cov"]).max() < 1e-4
    else:        # the gates of test_oracle_matches_reference
        assert d64 < 1e-4
        assert d32 < max(2e-4, float(np.abs(g["mean"] - g["mean64"]).max()) + 1e-4)
        assert np.abs(o["cov"] - g["cov64"]).max() / np.abs(g["cov64"]).max() < TOL_COV_REL
        assert np.abs(o["cov"] - g["cov"]).max() / np.abs(g["cov"]).max() < TOL_COV_REL
        assert np.abs(o["H_part1"] - g["H_part1_64"]).max() < 2e-5
        for lname in ("fc_block_4_mean", "fc_block_4_uncertainty"):      # the heads' raw outputs (before the 1e-3): L2 norm and 16 samples
            st, ref = o["layer_stats"][lname], g["L_" + lname]
            assert st[2] == ref[2] == 8 * n
            assert abs(st[1] - ref[1]) / ref[1] < 2e-5 and np.abs(st[3:] - ref[3:]).max() / np.abs(ref[3:]).max() < 1e-4, lname
    assert e64 < TOL_COV_ENTRY and e32 < TOL_COV_ENTRY
    assert hr.outside_blocks_zero(o["cov"]) and np.allclose(o["cov"], o["cov"].T, rtol=1e-6, atol=0)
    assert dms < 1e-4 and dlv < TOL_LOGVAR_S
    # the reference's own ensemble of its per-sample outputs is its covariance: the recorded samples and the recorded result belong together
    mean, cov, _ = hr.oracle_of().finish(g["mean_s"], g["logvar_s"], g["H_part1_64"])
    assert hr.cov_entry_err(cov, g["cov64"]) < TOL_COV_ENTRY and np.abs(mean - g["mean64"]).max() < 1e-4


def test_oracle_finish_against_a_numpy_restatement_at_wide_variances():
    """Oracle.finish is the reference of the GPU finish tests: here against numpy in float64 (model_to_trace.py:274-281 ensemble, :18-38 transfer
    cov = G diag(var_u, var_v) G^T with G = H[:2, :2] / (H[2] . p)), log-variances uniform in [-8, 8], a perspective H_part1"""
    from oracle import pyoracle
    rng = np.random.default_rng(7)
    p4 = np.array([0, 0, 0, 223, 319, 223, 319, 0], np.float64)
    for n in (1, 5, 16, 70):
        ms = (rng.standard_normal((n, 8)) * 5.0).astype(np.float32)
        lv = rng.uniform(-8.0, 8.0, (n, 8)).astype(np.float32)
        h = pyoracle.dlt((p4 + rng.uniform(-30.0, 30.0, 8)).astype(np.float32)).astype(np.float64)
        mean, cov, _ = hr.oracle_of().finish(ms, lv, h)
        mb = ms.astype(np.float64).mean(0)
        ens = ((mb - ms) ** 2).mean(0) + np.exp(lv.astype(np.float64)).mean(0)
        ref_mean, ref_cov = np.zeros(8), np.zeros((8, 8))
        for c in range(4):
            q = h @ np.array([p4[2 * c] + mb[2 * c], p4[2 * c + 1] + mb[2 * c + 1], 1.0])
            ref_mean[2 * c:2 * c + 2] = q[:2] / q[2] - p4[2 * c:2 * c + 2]
            g = h[:2, :2] / q[2]
            ref_cov[2 * c:2 * c + 2, 2 * c:2 * c + 2] = g @ np.diag(ens[2 * c:2 * c + 2]) @ g.T
        assert np.abs(mean - ref_mean).max() < 1e-4             # (the fp32 mean feeds the transfer: up to 5e-7 x |H| px)
        assert hr.cov_entry_err(cov, ref_cov) < 1e-6 and hr.outside_blocks_zero(cov)
