"""Every fp16-plane kernel (HNET_PREC_F16X2, csrc/s3_format.h) at the edges of the format's range, against the oracle's conv (double accumulation).

Operator level, one set of cases per kernel (tests/f16x2_range_cases.py builds them; tests/test_f16x2_range_cases_cpu.py checks their preconditions):
  A  inputs in the top binade of the guaranteed range (|a| up to 30000), ordinary outputs
  B  OUTPUTS in the top binade (matched patches); for the fused kernels the LDS-resident intermediate map (B) and then the output as well (B2)
  C  the band [32768, 65520) with planted near-tie values, whose second plane is an infinity: outputs no such input reaches are finite, and every
     finite output is at the fp32 level
  D  inputs in the fp16-subnormal range on zero biases: 2e-5 max |ref| + 2^-36 max_co sum |w_co|
The tolerance is the project's 2e-5 max |ref| throughout.  Forward level: per-layer weight gains put every layer's outputs at 24000 (tail chains, split-K
epilogues, fp32-output last layers, heads); then one interior layer x 4 leaves the range and the context must answer as HNET_PREC_BF16X3 does.
Each test prints `RANGE ...` lines with the worst error it saw: DESIGN.md keeps the table."""
import contextlib
import os

import numpy as np
import pytest

import f16x2_range_cases as rc

pytestmark = pytest.mark.gpu

PREC_BF16X3, PREC_F16X2 = 2, 3
ENV_KEYS = ("HNET_S3_TILE", "HNET_CHAIN", "HNET_FUSE_SMALL", "HNET_FUSE_B3", "HNET_FUSE_B42", "HNET_CHAIN_GRID", "HNET_CHAIN_FC", "HNET_WARP_FUSE",
            "HNET_GRAPH", "HNET_GRAPH_COPIES", "HNET_WARP_EXACT")
CONTEXTS = {"default": {}, "tile20": {"HNET_S3_TILE": "20"}, "tile21": {"HNET_S3_TILE": "21"}, "nochain": {"HNET_CHAIN": "0"}, "tile30": {"HNET_S3_TILE": "30"}}


@contextlib.contextmanager
def _env(values):
    """the kernel-selection variables HnetEngine maps onto hnet_config.variant: exactly `values`, nothing inherited, for the time of a create"""
    old = {k: os.environ.pop(k, None) for k in ENV_KEYS}
    os.environ.update(values)
    try:
        yield
    finally:
        for k in ENV_KEYS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def _engine(blob, ctx, precision=PREC_F16X2, max_batch=1, mc=4):
    from cuahn_vio_amd.homography_net import HnetEngine
    with _env(CONTEXTS[ctx]):
        return HnetEngine(blob, variant="full", mc_samples=mc, dropout_p=0.05, mc_seed=3, max_batch=max_batch, precision=precision)


@pytest.fixture(scope="module")
def engines(state):
    """engines by (weight set, context), created on first use: "plain" = the seed-0 weights, "zero_bias", "scaled2" (fused kernels' second layers scaled)"""
    from cuahn_vio_amd import weights
    made, blobs = {}, {}
    states = {"plain": lambda: state, "zero_bias": lambda: rc.zero_bias_state(state), "scaled2": lambda: rc.scaled_second_layers_state(state)}

    def get(wset, ctx):
        if (wset, ctx) not in made:
            if wset not in blobs:
                blobs[wset] = weights.pack_state_dict(states[wset]())
            e = _engine(blobs[wset], ctx)
            assert e.precision() == PREC_F16X2
            made[(wset, ctx)] = e
        return made[(wset, ctx)]
    yield get
    for e in made.values():
        e.close()


# (id, context, layer, batch, input size or None = the layer's size inside the network)
OPS = [(f"lean_l{l}", "tile20", l, 1, None) for l in (1, 2, 4, 6, 9, 10)] + [
    ("lean_l9_54x78", "tile20", 9, 1, (54, 78)),          # block_3_2 at 56 x 80 is the patch32 kernel in every context: off that size it is the lean kernel
    ("s3_l14", "tile20", 14, 1, None), ("s3_l8_21x27", "tile20", 8, 2, (21, 27)), ("s3_l15_19x23", "tile20", 15, 2, (19, 23)),
] + [(f"pipe_l{l}_b{b}", "tile21", l, b, None) for l in (4, 10, 5) for b in (1, 3)] + [
    (f"region_l{l}_b{b}", "tile21", l, b, None) for l in (1, 2, 6) for b in (1, 5)] + [
    ("patch_l8", "default", 8, 1, None), ("patch_l15", "default", 15, 1, None), ("patch32_l9", "default", 9, 1, None), ("first_s1_l7", "default", 7, 1, None),
] + [(f"first_s2_l{l}_b{b}", "default", l, b, None) for l in (0, 3) for b in (2, 17)]
CASES = ("A", "B", "C", "D")


def _report(op, case, rel, nonfinite):
    print(f"RANGE {op} case {case}: worst |hip - oracle| / max |oracle| = {rel:.2e}, non-finite outputs {100 * nonfinite:.3f} %")


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("op", OPS, ids=[o[0] for o in OPS])
def test_conv_kernel_at_the_edges_of_the_range(engines, state, op, case):
    name, ctx, layer, batch, size = op
    _n, cin, _cout, k, s, h, w = rc.geometry(layer)
    if size is not None:
        h, w = size
    wgt, bias = rc.weights_of(state, layer)
    rng = np.random.default_rng(1000 * layer + 10 * batch + CASES.index(case))
    shape = (batch, cin, h, w)
    touch = None
    if case == "A":
        x = rc.large_inputs(rng, shape)
    elif case == "B":
        x, _sites = rc.matched_patches(rng, wgt, s, shape)
    elif case == "C":
        x, mask = rc.near_tie_inputs(rng, shape)
        touch = rc.touched(mask, k, s, pad_cols=rc.PAIR_GEMM_PAD_COLS if layer == 7 else 0)
        assert mask.sum() >= 8 and touch.mean() <= 0.5
    else:
        x = rc.tiny_inputs(rng, shape)
        bias = np.zeros_like(bias)
    ref = rc.oracle_conv(x, wgt, bias, s)
    if case == "A":
        assert np.abs(x).max() < rc.RANGE and np.abs(ref).max() < rc.RANGE
    if case == "B":
        assert np.abs(x).max() < rc.RANGE and rc.in_top_binade(ref)
    got = engines("zero_bias" if case == "D" else "plain", ctx).op_conv(layer, x)
    bound = rc.tiny_bound(ref, wgt) if case == "D" else rc.TOL_REL * float(np.abs(ref).max())
    rel, nonfinite = rc.check_case(got, ref, bound, touch)
    _report(name, case, rel, nonfinite)
    if case == "C":
        assert nonfinite > 0, "an infinite second plane went through the kernel without a trace: was the planted value read?"


@pytest.mark.parametrize("case", ("A", "B", "B2", "C", "D"))
@pytest.mark.parametrize("which", sorted(rc.FUSED))
def test_fused_kernel_at_the_edges_of_the_range(engines, state, which, case):
    l1, l2 = rc.FUSED[which]
    _n, cin, _c, k1, s1, h, w = rc.geometry(l1)
    k2, s2 = rc.geometry(l2)[3:5]
    rng = np.random.default_rng(2000 + 10 * l1 + len(case) + ord(case[0]))
    shape = (1, cin, h, w)
    touch, gain2, st, wset = None, 1.0, state, "plain"
    if case == "A":
        x = rc.large_inputs(rng, shape)
    elif case in ("B", "B2"):
        x, g2 = rc.fused_matched_case(state, which)
        if case == "B2":
            gain2, wset = g2, "scaled2"
    elif case == "C":
        x, mask = rc.near_tie_inputs(rng, shape)
        touch = rc.touched(mask, k1, s1, k2, s2, pad_cols=rc.PAIR_GEMM_PAD_COLS if k1 == 7 else 0)
        assert mask.sum() >= 8 and touch.mean() <= 0.5
    else:
        x = rc.tiny_inputs(rng, shape)
        st, wset = rc.zero_bias_state(state), "zero_bias"
    mid, ref = rc.fused_oracle(st, which, x, gain2)
    if case != "C":
        assert np.abs(x).max() < rc.RANGE and np.abs(mid).max() < rc.RANGE and np.abs(ref).max() < rc.RANGE
    if case in ("B", "B2"):
        assert rc.in_top_binade(mid) and (case == "B" or rc.in_top_binade(ref))
    e = engines(wset, "default")
    got = {"block3": e.op_block3_fused, "block4": e.op_block4_fused, "block42": e.op_block42_fused}[which](x)
    bound = rc.tiny_bound(ref, rc.weights_of(st, l1)[0], rc.weights_of(st, l2)[0]) if case == "D" else rc.TOL_REL * float(np.abs(ref).max())
    rel, nonfinite = rc.check_case(got, ref, bound, touch)
    _report(which + "_fused", case, rel, nonfinite)
    if case == "C":
        assert nonfinite > 0


# ---- whole forwards -----------------------------------------------------------------------------------------------------------------------------
FWD_CONTEXTS = ("default", "nochain", "tile30")       # the tail chains; the per-layer launches with the last-arriver split-K epilogues; the reduce launches
N_MC, P_DROP, MC_SEED = 4, 0.05, 3


@pytest.fixture(scope="module")
def walk(state):
    """(gains, blob of the in-range weights, oracle answers of the two pairs, the float images)"""
    from cuahn_vio_amd import weights
    from oracle import pyoracle
    gains, _cum = rc.walk_gains(state)
    st = rc.scaled_state(state, gains)
    assert rc.max_conv_weight(st) < rc.WEIGHT_BOUND
    blob = weights.pack_state_dict(st)
    prev, curr = rc.walk_pairs()
    orc = pyoracle.Oracle(blob)
    ans = [orc.forward(prev[k], curr[k], n_mc=N_MC, p=P_DROP, mc_seed=MC_SEED, pair_seq=k) for k in range(2)]
    return gains, st, blob, ans, prev, curr


def _device_forward(e, prev, curr):
    """infer_batch_device on float images -> (mean [B, 8], overflow flag)"""
    import torch
    from cuahn_vio_amd.homography_net import PIX_F32
    dev = torch.device("cuda", 0)
    b = prev.shape[0]
    mean, cov = torch.zeros(b, 8, device=dev), torch.zeros(b, 64, device=dev)
    p, c = torch.from_numpy(prev).to(dev), torch.from_numpy(curr).to(dev)
    torch.cuda.synchronize()                   # the fills above run on torch's stream, the forward on the context's
    e.infer_batch_device(p.data_ptr(), c.data_ptr(), PIX_F32, None, b, 0, mean.data_ptr(), cov.data_ptr())
    flag = e.overflow_flag()
    return mean.cpu().numpy(), flag


@pytest.mark.parametrize("ctx", FWD_CONTEXTS)
def test_forward_with_every_layer_at_24000_stays_in_the_format(walk, ctx):
    from conftest import TOL_PX_VS_ORACLE
    gains, st, blob, ans, prev, curr = walk
    e = _engine(blob, ctx, max_batch=2, mc=N_MC)
    assert e.precision() == PREC_F16X2
    mean, cov = e.infer_batch(prev, curr, None)
    assert e.precision() == PREC_F16X2 and np.isfinite(mean).all() and np.isfinite(cov).all()
    worst = 0.0
    for pair in range(2):
        for blk, layers in rc.BLOCK_LAYERS.items():
            for la, lb in zip(layers[:-1], layers[1:]):
                w, b = rc.weights_of(st, lb)
                xin = e.debug_layer_output(la, pair)
                ref = rc.oracle_conv(xin[None], w, b, rc.geometry(lb)[4])[0]
                got = e.debug_layer_output(lb, pair)
                scale = float(np.abs(ref).max())
                assert 0.5 * rc.WALK_TARGET < scale < rc.RANGE, (lb, scale)
                err = float(np.abs(got.astype(np.float64) - ref).max()) / scale
                worst = max(worst, err)
                assert np.isfinite(got).all() and err < rc.TOL_REL, f"pair {pair} layer {lb}: {err:.3e}"
    m_dev, flag = _device_forward(e, prev, curr)
    assert flag == 0 and e.precision() == PREC_F16X2
    assert np.abs(m_dev - mean).max() < TOL_PX_VS_ORACLE
    e.close()
    d = max(float(np.abs(mean[k] - ans[k]["mean"]).max()) for k in range(2))
    e3 = _engine(blob, ctx, precision=PREC_BF16X3, max_batch=2, mc=N_MC)
    m3, _ = e3.infer_batch(prev, curr, None)
    e3.close()
    d3 = max(float(np.abs(m3[k] - ans[k]["mean"]).max()) for k in range(2))
    print(f"RANGE forward {ctx}: worst layer error {worst:.2e}; |mean - oracle| = {d:.2e} px (BF16X3 on the same weights: {d3:.2e} px), offsets up to "
          f"{max(np.abs(a['mean']).max() for a in ans):.1f} px")
    assert _gate(d, d3)


def _gate(d, d3):
    """|mean - oracle| of a forward: the project's gate, or twice what the BF16X3 context measures on the same weights where that is more"""
    from conftest import TOL_PX_VS_ORACLE
    return d < max(TOL_PX_VS_ORACLE, 2.0 * d3)


@pytest.mark.parametrize("layer", sorted(rc.BOOSTED), ids=[f"l{l}" for l in sorted(rc.BOOSTED)])
@pytest.mark.parametrize("ctx", FWD_CONTEXTS)
def test_one_interior_layer_out_of_range_is_detected_and_repaired(state, walk, ctx, layer):
    """one layer's gain x 4: its outputs pass 65520 while everything in front of it is in range.  Where those outputs live in fp16 planes the device
    entry point raises the flag and the host entry point answers exactly as a BF16X3 context, demoted.  The last layers of blocks 1 and 4
    (rc.IN_FP32) write fp32 for readers that take fp32: nothing overflows, the answer must be right as it stands"""
    from cuahn_vio_amd import weights
    from oracle import pyoracle
    gains, _st, _blob, _ans, prev, curr = walk
    st = rc.scaled_state(state, gains, (layer, 4.0))
    assert rc.max_conv_weight(st) < rc.WEIGHT_BOUND
    blob = weights.pack_state_dict(st)
    ref = _engine(blob, ctx, precision=PREC_BF16X3, max_batch=2, mc=N_MC)
    m_ref, c_ref = ref.infer_batch(prev, curr, None)
    ref.close()
    assert np.isfinite(m_ref).all() and np.isfinite(c_ref).all(), "the case must be finite in fp32-range arithmetic"
    e = _engine(blob, ctx, max_batch=2, mc=N_MC)
    assert e.precision() == PREC_F16X2
    _m, flag = _device_forward(e, prev, curr)
    prec_dev = e.precision()
    m, c = e.infer_batch(prev, curr, None)
    prec = e.precision()
    e.close()
    assert prec_dev == PREC_F16X2                      # the device path never switches the mode by itself
    if layer in rc.IN_FP32:
        orc = pyoracle.Oracle(blob)
        ans = [orc.forward(prev[k], curr[k], n_mc=N_MC, p=P_DROP, mc_seed=MC_SEED, pair_seq=k)["mean"] for k in range(2)]
        d, d3 = (max(float(np.abs(mm[k] - ans[k]).max()) for k in range(2)) for mm in (m, m_ref))
        print(f"RANGE forward {ctx}, {rc.BOOSTED[layer]} x 4: |mean - oracle| = {d:.2e} px (BF16X3: {d3:.2e} px), offsets up to {np.abs(ans).max():.1f} px")
        assert flag == 0 and prec == PREC_F16X2 and np.isfinite(m).all() and np.isfinite(c).all()
        assert _gate(d, d3)
        return
    assert flag == 1, "the device entry point did not raise hnet_overflow_flag"
    assert prec == PREC_BF16X3, "no demotion"
    assert np.array_equal(m, m_ref) and np.array_equal(c, c_ref)
