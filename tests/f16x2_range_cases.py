"""Shared by tests/test_f16x2_range_cases_cpu.py and tests/test_gpu_f16x2_kernel_range.py (not a test module): inputs that drive the fp16-plane
kernels (HNET_PREC_F16X2, csrc/s3_format.h) to the edges of the format's range, the numpy restatement of the activation split they are built
with, and the per-layer weight gains that put every layer of a whole forward into the top binade of the guaranteed range.

The format promises (csrc/s3_format.h): |a| < 32768 is carried at fp32 level; in [32768, 65520) a result is at fp32 level or non-finite; small
values lose only absolute precision, below 2^-37.  Every builder returns float32 arrays in the operators' NCHW layout; what each one guarantees
is asserted on the oracle's values by the CPU tests, and again by the GPU tests before they look at the device's answer."""
import numpy as np

TOL_REL = 2e-5                       # the project's element-wise gate: |hip - oracle| < 2e-5 max |oracle|
RANGE, F16_INF = 32768.0, 65520.0    # guaranteed range; first fp32 magnitude whose fp16 rounding is an infinity
TOP_BINADE = (16384.0, 32768.0)
MATCHED_TARGET = 28000.0             # output of a matched patch
LARGE_AMP = 30000.0
WALK_TARGET = 24000.0
IMAGE_GAIN = 4096.0                  # the forward cases feed float images x 4096 (exact): with images in [0, 1] the first layer of a block would need
                                     # a gain of ~5e4 (weights of ~5e3, far beyond the format's |w| < 16) to reach 24000
WEIGHT_BOUND = 15.99                 # cuahn_vio_amd.weights.F16X2_WEIGHT_BOUND

BLOCK_SIZE = {1: (28, 40), 2: (56, 80), 3: (112, 160), 4: (224, 320)}
BLOCK_LAYERS = {1: (0, 1, 2), 2: (3, 4, 5, 6), 3: (7, 8, 9, 10, 11, 12), 4: (13, 14, 15, 16, 17, 18, 19)}
FC_OF_BLOCK = {1: ("model_part1.fc_block_1",), 2: ("model_part1.fc_block_2",), 3: ("model_part1.fc_block_3",),
               4: ("model_last_block_list.0.fc_block_4_mean.1", "model_last_block_list.0.fc_block_4_uncertainty.1")}


# ---- the format ---------------------------------------------------------------------------------------------------------------------------------
def split2h_np(v):
    """hnet::split2h with numpy casts: (A0, A1) float16 arrays, A0 = f16(v), A1 = f16((v - A0) 4096); overflow goes to an infinity"""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        a0 = v.astype(np.float16)
        a1 = ((v - a0.astype(np.float32)) * np.float32(4096.0)).astype(np.float16)
    return a0, a1


def infinite_second_plane(x):
    """elements whose first plane is finite and whose second is not: the near-tie values of [32768, 65520)"""
    a0, a1 = split2h_np(x)
    return np.isfinite(a0) & ~np.isfinite(a1)


def near_tie_values(rng, n):
    """n fp32 values of [32768, 65520) within 2^-8 of the rounding tie between two fp16 neighbours (fp16 ulp 32 there, ties at 32784 + 32 k): the
    tie itself and its two fp32 neighbours.  Their residual is >= 16 - 2^-8, x 4096 >= 65520: an infinite second plane"""
    tie = 32784.0 + 32.0 * rng.integers(0, 1023, n)
    return (tie + rng.integers(-1, 2, n) * 2.0 ** -8).astype(np.float32)


# ---- layers -------------------------------------------------------------------------------------------------------------------------------------
def geometry(layer):
    """(name, cin, cout, k, stride, h, w): conv layer `layer` with the input size it has inside the network"""
    from cuahn_vio_amd.weights import CONV_LAYERS
    name, cin, cout, k, s = CONV_LAYERS[layer]
    h, w = BLOCK_SIZE[int(name[6])]
    for n2, _ci, _co, k2, s2 in CONV_LAYERS:
        if n2 == name:
            break
        if n2[6] == name[6]:
            h, w = out_size(h, w, k2, s2)
    return name, cin, cout, k, s, h, w


def out_size(h, w, k, s):
    p = (k - 1) // 2
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


def key_of(layer):
    from cuahn_vio_amd.weights import CONV_LAYERS
    name = CONV_LAYERS[layer][0]
    return ("model_last_block_list.0." if name[6] == "4" else "model_part1.") + name + ".0"


def weights_of(state, layer):
    k = key_of(layer)
    return state[k + ".weight"], state[k + ".bias"]


def matched_gain(w):
    """sum |w| per output channel: the output of a patch x = amp sign(w[co]) is amp times this"""
    return np.abs(np.asarray(w, np.float64)).reshape(w.shape[0], -1).sum(1)


def zero_bias_state(state):
    """a copy with every convolution's bias zeroed (the tiny-input cases: a bias of O(0.1) would hide outputs of O(1e-5))"""
    st = {k: v.copy() for k, v in state.items()}
    for k in st:
        if ".block_" in k and k.endswith(".0.bias"):
            st[k][...] = 0
    return st


def oracle_conv(x, w, b, s):
    """pyoracle.conv_lrelu over a batch: [B, Cin, H, W] -> [B, Cout, Ho, Wo]"""
    from oracle import pyoracle
    return np.stack([pyoracle.conv_lrelu(xb, w, b, s) for xb in x])


# ---- input builders -----------------------------------------------------------------------------------------------------------------------------
def large_inputs(rng, shape, amp=LARGE_AMP):
    """ordinary activations with 2 % of the elements at +-(0.6 .. 1.0) amp: the INPUT planes are probed, the outputs stay far inside the range"""
    x = rng.standard_normal(shape).astype(np.float32)
    big = rng.random(shape) < 0.02
    n = int(big.sum())
    x[big] = (rng.uniform(0.6, 1.0, n) * amp * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    return x


def matched_sites(h, w, k, s, n):
    """up to n output positions whose receptive fields lie inside the image and do not overlap, spread over the map"""
    p = (k - 1) // 2
    ho, wo = out_size(h, w, k, s)
    d = -(-k // s)
    oys = [oy for oy in range(ho) if oy * s - p >= 0 and oy * s - p + k <= h][::d]
    oxs = [ox for ox in range(wo) if ox * s - p >= 0 and ox * s - p + k <= w][::d]
    sites = [(oy, ox) for oy in oys for ox in oxs]
    if len(sites) <= n:
        return sites
    return [sites[round(i * (len(sites) - 1) / (n - 1))] for i in range(n)] if n > 1 else sites[:1]


def matched_patches(rng, w, s, shape, target=MATCHED_TARGET, noise=0.1, n_sites=3):
    """x = noise N(0, 1) with x[b, :, patch] = amp sign(w[co]) at n_sites output positions per batch element, amp = target / sum |w[co]|: the output
    channel co at that position is ~ target, every input stays below target / min gain.  The channels: smallest gain (largest input), largest gain,
    and others in turn.  -> (x, [(b, co, oy, ox)])"""
    b_n, cin, h, wd = shape
    cout, _cin, k, _k = w.shape
    p = (k - 1) // 2
    g = matched_gain(w)
    order = [int(np.argmin(g)), int(np.argmax(g))] + [int(c) for c in rng.permutation(cout)]
    x = (rng.standard_normal(shape) * noise).astype(np.float32)
    sites = []
    for b in range(b_n):
        for i, (oy, ox) in enumerate(matched_sites(h, wd, k, s, n_sites)):
            co = order[(i + b) % len(order)]
            y0, x0 = oy * s - p, ox * s - p
            x[b, :, y0:y0 + k, x0:x0 + k] = (np.sign(w[co]) * (target / g[co])).astype(np.float32)
            sites.append((b, co, oy, ox))
    return x, sites


def near_tie_inputs(rng, shape, n_plant=8):
    """ordinary activations, 2 % of the elements at ordinary values of the band [32768, 65520), and per batch element n_plant near-tie values
    (second plane infinite) on a 2 x 2 block of pixels in the middle of the map -> (x, mask of the elements whose second plane is infinite).  Random
    band values qualify with probability 3.7e-4 (3 of the 8192 fp32 values per fp16 ulp): they must be planted; the mask holds every one, planted or
    drawn"""
    b_n, cin, h, w = shape
    x = rng.standard_normal(shape).astype(np.float32)
    band = rng.random(shape) < 0.02
    n = int(band.sum())
    x[band] = (rng.uniform(RANGE, F16_INF - 1.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    per_pix = -(-n_plant // 4)
    y0, x0 = max(h // 2 - 1, 0), max(w // 2 - 1, 0)
    for b in range(b_n):
        for dy in range(2):
            for dx in range(2):
                ch = rng.choice(cin, min(per_pix, cin), replace=False)
                x[b, ch, min(y0 + dy, h - 1), min(x0 + dx, w - 1)] = near_tie_values(rng, len(ch)) * rng.choice([-1.0, 1.0], len(ch))
    return x, infinite_second_plane(x)


def tiny_inputs(rng, shape):
    """N(0, 1) 2^-16: the first plane is an fp16 subnormal (|v| < 2^-14 up to 4 sigma)"""
    return (rng.standard_normal(shape) * 2.0 ** -16).astype(np.float32)


def tiny_bound(ref, *ws):
    """case D: 2e-5 max |ref| + 2^-36 max_co sum |w_co| for one layer.  An activation in the fp16-subnormal range is carried to 2^-37 absolute (both
    planes sit on grids of 2^-24 and 2^-36); the factor 2 covers the LeakyReLU and the dropped A1 W1 term.  Two fused layers (w1, w2): the first
    layer's absolute error e1 = 2^-36 G1 enters the second through its weights, the second adds its own: 2^-36 G2 (1 + G1), G = max_co sum |w_co|"""
    g = [float(matched_gain(w).max()) for w in ws]
    a = g[0] if len(g) == 1 else g[1] * (1.0 + g[0])
    return TOL_REL * float(np.abs(ref).max()) + 2.0 ** -36 * a


def touched(mask, k, stride, k2=None, stride2=None, pad_cols=0):
    """outputs whose receptive field contains a masked input: mask [B, C, H, W] or [B, H, W] -> bool [B, Ho, Wo] (every output channel alike);
    with k2, stride2: through a second layer on top of the first.  pad_cols widens the FIRST layer's window by that many columns on either side:
    what a kernel reads beyond the receptive field with zero weights (PAIR_GEMM_PAD_COLS) - an infinite plane times zero is a NaN"""
    m = np.asarray(mask, bool)
    if m.ndim == 4:
        m = m.any(1)
    p = (k - 1) // 2
    b, h, w = m.shape
    ho, wo = out_size(h, w, k, stride)
    mp = np.zeros((b, h + 2 * p, w + 2 * p + 2 * pad_cols), bool)
    mp[:, p:p + h, p + pad_cols:p + pad_cols + w] = m
    out = np.zeros((b, ho, wo), bool)
    for kh in range(k):
        for kw in range(k + 2 * pad_cols):
            out |= mp[:, kh:kh + (ho - 1) * stride + 1:stride, kw:kw + (wo - 1) * stride + 1:stride]
    return touched(out, k2, stride2) if k2 is not None else out


# The 7 x 7 stride-1 layers on two input channels (block_3_0, block_4_0; conv_first.h, conv_b3_fused.h, conv_b4_fused.h) are pixel-pair GEMMs: two
# adjacent output pixels share ONE operand row K = (kh, kw' 0..7, ci) of eight input columns, the eighth tap of either pixel carrying a zero weight.
# An output at column x so reads column x + 4 or x - 4 (by its place in the pair) on top of x - 3 .. x + 3; the band cases take both.
PAIR_GEMM_PAD_COLS = 1


def check_case(got, ref, bound, touch=None):
    """the assertion of every operator case.  got, ref [B, C, H, W]; touch [B, H, W] or None.  Outside `touch` every output is finite; every finite
    output is within `bound` of the oracle.  -> (worst |got - ref| / max |ref| of the finite outputs, share of non-finite outputs)"""
    fin = np.isfinite(got)
    outside = np.ones(got.shape, bool) if touch is None else np.broadcast_to(~touch[:, None], got.shape)
    assert fin[outside].all(), f"{int((~fin[outside]).sum())} non-finite outputs that no out-of-range input reaches"
    err = float(np.abs(got[fin].astype(np.float64) - ref[fin]).max())
    assert err <= bound, f"max |hip - oracle| = {err:.3e} > {bound:.3e} (max |oracle| = {np.abs(ref).max():.3e})"
    return err / float(np.abs(ref).max()), float(1.0 - fin.mean())


def in_top_binade(a):
    m = float(np.abs(a).max())
    return TOP_BINADE[0] <= m < TOP_BINADE[1]


# ---- whole forwards: per-layer weight gains -------------------------------------------------------------------------------------------------------
_cache = {}


def walk_pairs():
    """the two pairs of the forward cases as float images x IMAGE_GAIN: (prev [2, 224, 320] float32, curr)"""
    from cuahn_vio_amd import synth
    from oracle import pyoracle
    if "pairs" not in _cache:
        ps = [synth.make_pair(s)[:2] for s in (21, 22)]
        f = lambda i: np.stack([pyoracle.as_f32_image(p[i]) * np.float32(IMAGE_GAIN) for p in ps])
        _cache["pairs"] = (f(0), f(1))
    return _cache["pairs"]


def layer_maxima(state, img1, img2):
    """max |output| of each of the 20 conv layers on one float pair, with pyoracle's operators (double accumulation) chained as oracle_forward
    chains them; the corner targets of blocks 1 - 3 come from the oracle's own trace -> (maxima [20], feat [5120], the trace)"""
    from cuahn_vio_amd import weights
    from oracle import pyoracle
    tr = pyoracle.Oracle(weights.pack_state_dict(state)).forward(img1, img2, n_mc=1, p=0.0, want_trace=True)
    mx = np.zeros(20)
    hm = np.eye(3, dtype=np.float32)
    x = None
    for blk in (1, 2, 3, 4):
        warped = img2 if blk == 1 else pyoracle.warp(img2, hm)
        x = np.stack([img1, warped]).astype(np.float32)
        if blk < 4:
            x = pyoracle.avgpool(x, 224 // BLOCK_SIZE[blk][0])
        for l in BLOCK_LAYERS[blk]:
            w, b = weights_of(state, l)
            x = pyoracle.conv_lrelu(x, w, b, geometry(l)[4])
            mx[l] = np.abs(x).max()
        if blk < 4:
            hb = pyoracle.dlt(tr["dlt_dst"][blk - 1])
            hm = hb if blk == 1 else (hm.astype(np.float64) @ hb.astype(np.float64)).astype(np.float32)
    return mx, x.reshape(-1), tr


def walk_gains(state, target=WALK_TARGET):
    """weight gain per conv layer so that the layer's largest output over walk_pairs() is `target`.  The network is positively homogeneous (the
    biases scaled along), so the walk is one pass of the unscaled network over the images in [0, 1]: with C_l = target / max_l the layer's weights
    take C_l / C_(l-1) (in front of a block: C = IMAGE_GAIN, the images' own factor) and its bias C_l; every activation of the scaled network on
    the scaled images is then C_l times the unscaled one, and with the 5120-input FC weights divided by the last C of their block (as
    weights.variant_state does) the corner offsets, hence the warps, are those of the unscaled network.  -> gains [20], cumulative C [20]"""
    if "gains" not in _cache:
        prev, curr = walk_pairs()
        unit = np.float32(1.0 / IMAGE_GAIN)
        mx = np.maximum(layer_maxima(state, prev[0] * unit, curr[0] * unit)[0], layer_maxima(state, prev[1] * unit, curr[1] * unit)[0])
        cum = target / mx
        g = cum / IMAGE_GAIN
        for blk, layers in BLOCK_LAYERS.items():
            for a, b in zip(layers[:-1], layers[1:]):
                g[b] = cum[b] / cum[a]
        _cache["gains"] = (g, cum)
    return _cache["gains"]


def scaled_state(state, gains, boost=None):
    """the state dict with layer l's weights x gains[l] and its bias x the cumulative gain, the FC layers behind each block divided by the block's
    cumulative gain.  boost = (layer, factor): that layer's weights and bias times factor on top, nothing else changed - the layer's outputs, and
    everything behind it, grow by the factor"""
    st = {k: v.copy() for k, v in state.items()}
    for blk, layers in BLOCK_LAYERS.items():
        c = IMAGE_GAIN
        for l in layers:
            c *= gains[l]
            f = boost[1] if boost is not None and boost[0] == l else 1.0
            k = key_of(l)
            st[k + ".weight"] = (st[k + ".weight"].astype(np.float64) * gains[l] * f).astype(np.float32)
            st[k + ".bias"] = (st[k + ".bias"].astype(np.float64) * c * f).astype(np.float32)
        for fc in FC_OF_BLOCK[blk]:
            st[fc + ".weight"] = (st[fc + ".weight"].astype(np.float64) / c).astype(np.float32)
    return st


def max_conv_weight(state):
    return max(float(np.abs(weights_of(state, l)[0]).max()) for l in range(20))


def second_layer_gain(out, target=MATCHED_TARGET):
    """factor on a fused kernel's second-layer weights that lifts the largest output (of the unscaled second layer) to `target`"""
    return target / float(np.abs(out).max())


# the layers whose gain the out-of-range forward cases multiply by 4, one at a time.  The last layer of a block writes fp32 (the block-tail FC and the
# heads read fp32 features, the heads scale them into the planes' range: capi_weights.hip), so ITS outputs beyond 65520 leave no fp16 plane: those two
# cases (IN_FP32) must give the right answer without a demotion; the layers in front of them make the last layer's INPUT planes overflow instead
BOOSTED = {13: "block_4_0 (the fused kernel's LDS-resident map)", 7: "block_3_0", 5: "block_2_3 (inside a tail chain)",
           1: "block_1_2 (block_1_3 turns it into non-finite features for FC -> DLT -> warp)", 2: "block_1_3 (feeds FC -> DLT -> warp)",
           18: "block_4_5 (block_4_6 turns it into non-finite features for the heads)", 19: "block_4_6 (feeds the heads)"}
IN_FP32 = (2, 19)


# ---- the fused kernels' cases -----------------------------------------------------------------------------------------------------------------------
FUSED = {"block3": (7, 8), "block4": (13, 14), "block42": (15, 16)}      # (first layer, second layer) of op_block3_fused / op_block4_fused / op_block42_fused


def fused_oracle(state, which, x, gain2=1.0):
    """(intermediate map, output) of the oracle's two layers; gain2 multiplies the second layer's weights"""
    l1, l2 = FUSED[which]
    (w1, b1), (w2, b2) = weights_of(state, l1), weights_of(state, l2)
    mid = oracle_conv(x, w1, b1, geometry(l1)[4])
    return mid, oracle_conv(mid, w2 * np.float32(gain2), b2, geometry(l2)[4])


def fused_matched_case(state, which):
    """the first-layer matched patches of a fused kernel (batch 1) and the second-layer gain that lifts the output to MATCHED_TARGET as well
    -> (x, gain2)"""
    key = ("fused", which)
    if key not in _cache:
        l1 = FUSED[which][0]
        _n, cin, _c, _k, s1, h, w = geometry(l1)
        x, _sites = matched_patches(np.random.default_rng(50 + l1), weights_of(state, l1)[0], s1, (1, cin, h, w))
        x.setflags(write=False)
        _cache[key] = (x, second_layer_gain(fused_oracle(state, which, x)[1]))
    return _cache[key]


def scaled_second_layers_state(state):
    """a copy with the second layer of every fused kernel scaled by its fused_matched_case gain"""
    st = {k: v.copy() for k, v in state.items()}
    for which, (_l1, l2) in FUSED.items():
        k = key_of(l2) + ".weight"
        st[k] = st[k] * np.float32(fused_matched_case(state, which)[1])
    return st
