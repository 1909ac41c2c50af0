"""tests/f16x2_range_cases.py on the CPU: the numpy restatement of the activation split against hnet::split2h bit for bit, every input builder's
preconditions on the oracle's values, `touched` against a brute-force convolution of the mask, and the per-layer weight gains of the forward cases
(tests/test_gpu_f16x2_kernel_range.py runs them on the device)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import f16x2_range_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_split2h_np_is_split2h_bit_for_bit(tmp_path):
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(clang):
        clang = shutil.which("hipcc")
    if not clang:
        pytest.skip("no HIP compiler on this machine (the header includes hip_runtime.h)")
    exe = str(tmp_path / "split2h_print.bin")
    subprocess.run([clang, "-O2", "-x", "hip", "--offload-host-only", "-I" + ROOT, "-I/opt/rocm/include", "-w",
                    os.path.join(ROOT, "tests", "cpp", "split2h_print.cpp"), "-o", exe], check=True, timeout=300)
    rng = np.random.default_rng(11)
    n = 1_000_000
    sign = lambda k: rng.choice([-1.0, 1.0], k)
    ties = rc.near_tie_values(rng, 4096) * sign(4096)
    bands = {
        "subnormal first plane": rng.standard_normal(n) * 2.0 ** -16,
        "below fp16's smallest subnormal": rng.standard_normal(n) * 2.0 ** -27,
        "ordinary": rng.standard_normal(n) * rng.choice([1e-3, 1.0, 300.0], n),
        "top binade of the range": rng.uniform(16384.0, 32768.0, n) * sign(n),
        "band": rng.uniform(32768.0, 65520.0, n) * sign(n),
        "beyond": rng.uniform(65520.0, 1.0e6, n) * sign(n),
        "planted ties": ties,
        "edges": np.array([0.0, -0.0, 2.0 ** -24, 2.0 ** -25, 2.0 ** -14, 32767.998, 32768.0, 65519.996, 65520.0, 65504.0, np.inf, -np.inf]),
    }
    v = np.concatenate([b.astype(np.float32) for b in bands.values()])
    v.tofile(str(tmp_path / "in.f32"))
    subprocess.run([exe, str(tmp_path / "in.f32"), str(tmp_path / "out.u16")], check=True, timeout=120)
    host = np.fromfile(str(tmp_path / "out.u16"), np.uint16).reshape(-1, 2)
    a0, a1 = rc.split2h_np(v)
    nan = np.isnan(a1)                                     # (A0 infinite: the residual is inf - inf on both sides; only the payload may differ)
    assert np.array_equal(a0.view(np.uint16), host[:, 0])
    assert np.array_equal(a1.view(np.uint16)[~nan], host[~nan, 1])
    assert ((host[nan, 1] & 0x7FFF) > 0x7C00).all()
    # and the band is what the format's header says: an infinite second plane for about 3 of 8192 values, for every planted one, never below 32768
    pos = 0
    share = {}
    for name, b in bands.items():
        share[name] = float(rc.infinite_second_plane(v[pos:pos + len(b)]).mean())
        pos += len(b)
    print({k: f"{s:.5f}" for k, s in share.items()})
    assert share["planted ties"] == 1.0 and share["top binade of the range"] == 0.0 and share["ordinary"] == 0.0
    assert 2.0e-4 < share["band"] < 6.0e-4


OP_LAYERS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 14, 15]


@pytest.mark.parametrize("layer", OP_LAYERS)
def test_builders_meet_their_preconditions_on_the_oracle(state, layer):
    name, cin, cout, k, s, h, w = rc.geometry(layer)
    wgt, bias = rc.weights_of(state, layer)
    rng = np.random.default_rng(layer)
    shape = (2, cin, h, w)
    # A: inputs at the edge, outputs inside
    x = rc.large_inputs(rng, shape)
    assert 0.9 * rc.LARGE_AMP < np.abs(x).max() < rc.RANGE
    assert np.abs(rc.oracle_conv(x, wgt, bias, s)).max() < rc.RANGE
    # B: outputs at the edge, inputs inside
    x, sites = rc.matched_patches(rng, wgt, s, shape)
    ref = rc.oracle_conv(x, wgt, bias, s)
    assert len(sites) >= 2 and np.abs(x).max() < rc.RANGE and rc.in_top_binade(ref)
    for b, co, oy, ox in sites:
        assert abs(ref[b, co, oy, ox] - rc.MATCHED_TARGET) < 0.02 * rc.MATCHED_TARGET
    # C: the band; at least 8 planted near ties per batch element, every one in the mask, at most half of the outputs reached
    x, mask = rc.near_tie_inputs(rng, shape)
    assert np.abs(x).max() < rc.F16_INF and np.isfinite(rc.split2h_np(x)[0]).all()
    assert (mask.reshape(2, -1).sum(1) >= 8).all() and (np.abs(x[mask]) >= rc.RANGE).all()
    assert ((np.abs(x) >= rc.RANGE) & ~mask).sum() > mask.sum()             # ordinary band values around them
    t = rc.touched(mask, k, s)
    assert 0 < t.mean() <= 0.5
    ref = rc.oracle_conv(x, wgt, bias, s)
    assert np.abs(ref[np.broadcast_to(~t[:, None], ref.shape)]).max() < rc.RANGE      # the outputs no near tie reaches stay inside the guaranteed range
    # D: first plane an fp16 subnormal
    x = rc.tiny_inputs(rng, shape)
    a0 = np.abs(rc.split2h_np(x)[0].astype(np.float32))
    assert (a0 < 2.0 ** -14).mean() > 0.999 and (a0 > 0).mean() > 0.9
    ref = rc.oracle_conv(x, wgt, np.zeros_like(bias), s)
    assert 2.0 ** -36 * rc.matched_gain(wgt).max() < rc.tiny_bound(ref, wgt) < 1e-3 * np.abs(ref).max()      # the bound still resolves the outputs


@pytest.mark.parametrize("which", sorted(rc.FUSED))
def test_fused_cases_put_the_intermediate_map_and_the_output_at_the_edge(state, which):
    l1, l2 = rc.FUSED[which]
    _n, cin, _c, k1, s1, h, w = rc.geometry(l1)
    s2 = rc.geometry(l2)[4]
    (w1, b1), (w2, b2) = rc.weights_of(state, l1), rc.weights_of(state, l2)
    rng = np.random.default_rng(60 + l1)
    x, g2 = rc.fused_matched_case(state, which)
    mid, out = rc.fused_oracle(state, which, x)
    assert np.abs(x).max() < rc.RANGE and rc.in_top_binade(mid) and np.abs(out).max() < rc.RANGE
    assert np.abs(rc.weights_of(rc.scaled_second_layers_state(state), l2)[0]).max() < rc.WEIGHT_BOUND
    mid2, out2 = rc.fused_oracle(state, which, x, g2)
    assert np.array_equal(mid, mid2) and rc.in_top_binade(out2)
    # A and C through two layers
    assert np.abs(rc.oracle_conv(rc.large_inputs(rng, x.shape), w1, b1, s1)).max() < rc.RANGE
    xc, mask = rc.near_tie_inputs(rng, x.shape)
    midc = rc.oracle_conv(xc, w1, b1, s1)
    assert np.abs(midc[np.broadcast_to(~rc.touched(mask, k1, s1)[:, None], midc.shape)]).max() < rc.RANGE
    assert 0 < rc.touched(mask, k1, s1, w2.shape[2], s2).mean() <= 0.5


@pytest.mark.parametrize("k,s,hw", [(3, 2, (7, 10)), (5, 2, (14, 20)), (7, 1, (12, 9)), (7, 2, (28, 40)), (3, 2, (6, 7))])
def test_touched_is_a_convolution_of_the_mask(k, s, hw):
    from oracle import pyoracle
    rng = np.random.default_rng(k * 10 + s)
    mask = rng.random((2, 3) + hw) < 0.03
    mask[0, 0, 0, 0] = mask[1, 2, -1, -1] = True             # the corners: padding on two sides
    zero = np.zeros(1, np.float32)
    conv = lambda m, kk, ss: np.stack([pyoracle.conv_lrelu(mb[None].astype(np.float32), np.ones((1, 1, kk, kk), np.float32), zero, ss)[0] > 0 for mb in m])
    brute = conv(mask.any(1), k, s)
    got = rc.touched(mask, k, s)
    assert got.dtype == bool and np.array_equal(got, brute)
    assert np.array_equal(rc.touched(mask, k, s, 5, 2), conv(brute, 5, 2))
    # pad_cols: the window one column wider on either side = the mask, or its copies moved one column left and right, inside the plain window
    m2 = mask.any(1)
    wide = m2.copy()
    wide[:, :, 1:] |= m2[:, :, :-1]
    wide[:, :, :-1] |= m2[:, :, 1:]
    if s == 1:
        assert np.array_equal(rc.touched(mask, k, s, pad_cols=1), conv(wide, k, s))


def test_walk_gains_put_every_layer_at_24000_with_weights_inside_the_format(state):
    """the restated chain of pyoracle operators is oracle_forward's (same features); on the scaled weights every layer's largest output over the two
    pairs is 24000, every |w| < 16, the corner offsets are those of the unscaled network; one layer x 4 leaves the format's range, its inputs do not"""
    from cuahn_vio_amd import weights
    from oracle import pyoracle
    prev, curr = rc.walk_pairs()
    mx0, feat, tr = rc.layer_maxima(state, prev[0], curr[0])
    assert np.array_equal(feat, tr["feat"])
    gains, cum = rc.walk_gains(state)
    st = rc.scaled_state(state, gains)
    assert rc.max_conv_weight(st) < rc.WEIGHT_BOUND and 4.0 * rc.max_conv_weight(st) < rc.WEIGHT_BOUND
    mx = np.maximum(rc.layer_maxima(st, prev[0], curr[0])[0], rc.layer_maxima(st, prev[1], curr[1])[0])
    print("gains", np.round(gains, 3), "largest outputs", np.round(mx))
    assert np.abs(mx / rc.WALK_TARGET - 1.0).max() < 1e-3
    unit = np.float32(1.0 / rc.IMAGE_GAIN)
    o0 = pyoracle.Oracle(weights.pack_state_dict(state)).forward(prev[0] * unit, curr[0] * unit, n_mc=4, p=0.05, mc_seed=3, pair_seq=0)
    o1 = pyoracle.Oracle(weights.pack_state_dict(st)).forward(prev[0], curr[0], n_mc=4, p=0.05, mc_seed=3, pair_seq=0)
    assert np.abs(o0["mean"]).max() > 1.0 and np.abs(o1["mean"] - o0["mean"]).max() < 1e-3
    for layer in rc.BOOSTED:
        b = rc.layer_maxima(rc.scaled_state(state, gains, (layer, 4.0)), prev[0], curr[0])[0]
        assert b[layer] > rc.F16_INF and (b[:layer] < rc.RANGE).all()
