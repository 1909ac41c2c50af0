"""What synthetic texture says about cov_scale (include/hnet.h hnet_filters_set_photo_refine).  Recorded, not gated, and NOT a calibration for
flight footage: the 16 pairs are the accuracy rows of DESIGN 7n (tests/photo_robust_util.py ROWS: stock and basin pairs of seeds 1, 2, 5, 11 with an
exposure step, half of them with a foreign block), synthetic texture warped by a known homography.  Per pair hnet_op_photo_align_robust runs with the
row's own levels and trials on the GPU; from its level-0 record R = mse * inverse(info8) (cov_scale = 1, no floor; info8 = hnet_photo_robust_marginal) is
formed in float64, and err_i^2 / R_ii printed for the eight offsets (1 on average for a calibrated covariance).  Then the scale that brings their mean
to 1, without a floor and with the default 0.05 px floor.
   python tools/photo_refine_calibrate.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import photo_robust_util as R
    from cuahn_vio_amd import _capi, weights
    from cuahn_vio_amd.homography_net import HnetEngine
    e = HnetEngine(weights.pack_state_dict(weights.synthetic_state(0)), variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=1, max_batch=8)
    err2, var = [], []
    for name in R.ROWS:
        levels, kw = R.row_opts(name)
        i1, i2, truth, start = R.row_pairs(name)
        out = e.op_photo_align_robust(i1, i2, start, levels=levels, **kw)
        for k, seed in enumerate((1, 2, 5, 11)):
            info8, _ = _capi.photo_robust_marginal(out[k])
            v = float(out[k]["px"]["mse"]) * np.diag(np.linalg.inv(info8))
            d2 = (out[k]["px"]["offsets_px"].astype(np.float64) - truth[k]) ** 2
            err2.append(d2)
            var.append(v)
            print(f"{name:14s} seed {seed:2d}: worst {np.sqrt(d2.max()):.4f} px off, mse {out[k]['px']['mse']:8.3f}, sqrt(R_ii) {np.sqrt(v).round(4)}, "
                  f"err_i^2 / R_ii {np.array2string(d2 / v, precision=2, suppress_small=True)}  mean {np.mean(d2 / v):.2f}")
    err2, var = np.array(err2), np.array(var)
    ratio = err2 / var
    print(f"all 16 pairs x 8 offsets at cov_scale = 1, no floor: mean err^2 / R_ii = {ratio.mean():.2f}, median {np.median(ratio):.2f}, max {ratio.max():.1f}")
    print(f"  per row: " + ", ".join(f"{name} {ratio[4 * k:4 * k + 4].mean():.2f}" for k, name in enumerate(R.ROWS)))
    print(f"cov_scale that brings the mean to 1 without a floor: {ratio.mean():.2f}")
    floor2 = 0.05 ** 2
    mean_at = lambda s: float((err2 / (s * var + floor2)).mean())
    if mean_at(0.0) <= 1.0:
        print(f"with the default floor of 0.05 px the mean is {mean_at(0.0):.2f} <= 1 at cov_scale -> 0: on these pairs the floor alone covers the error")
    else:
        lo, hi = 0.0, 1.0
        while mean_at(hi) > 1.0:
            hi *= 2.0
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if mean_at(mid) > 1.0 else (lo, mid)
        print(f"cov_scale that brings the mean to 1 with the default floor of 0.05 px: {hi:.2f} (mean at cov_scale = 1: {mean_at(1.0):.2f})")
    print("synthetic texture with independent pixel noise only from rounding: no statement about flight footage")
    e.close()


if __name__ == "__main__":
    main()
