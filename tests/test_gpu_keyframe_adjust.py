"""The joint adjustment of a keyframe map on the device, operator level (include/hnet.h hnet_op_keyframe_adjust_solve, hnet_op_keyframe_adjust;
csrc/kernels_keyframe_adjust.hip): the solve byte for byte the host reference's (tests/cpp/keyframe_adjust_ref.cpp compiles the header the
device compiles), the whole call on the texture map of the render's tests - its table, its alignment records, its record against the header on the
device's own records and against the wholly-host reference, the size of the correction and the render after it -, a drifted loop against the truth, a
map whose 28 jobs take four rounds, and the refusals.  A context of max_batch 8."""
import ctypes as C

import numpy as np
import pytest

import keyframe_adjust_util as A
import keyframe_render_util as R
from cuahn_vio_amd import _capi

pytestmark = pytest.mark.gpu

INVALID = 1
UNIT, INFO = _capi.ADJ_WEIGHT_UNIT, _capi.ADJ_WEIGHT_INFO
ADJUSTED = _capi.ADJ_ADJUSTED


@pytest.fixture(scope="module")
def aref(tmp_path_factory):
    return A.build_ref(tmp_path_factory.mktemp("keyframe_adjust_ref_gpu"))


@pytest.fixture(scope="module")
def eng(blob):
    from cuahn_vio_amd.homography_net import HnetEngine
    e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=8)
    yield e
    e.close()


def _same(dev, ref, what):
    if dev.tobytes() != ref.tobytes():
        bad = [f for f in A.REC.names if np.asarray(dev[0][f]).tobytes() != np.asarray(ref[0][f]).tobytes()]
        raise AssertionError((what, bad, dev[0]["flags"], ref[0]["flags"], dev[0]["trials"], ref[0]["trials"], dev[0]["cost"], ref[0]["cost"]))


def _infos(n, seed):
    """symmetric positive definite 8 x 8 matrices of the size an alignment's information has"""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(n, 8, 8))
    return (a @ a.transpose(0, 2, 1) + 8.0 * np.eye(8)) * 50.0


@pytest.mark.parametrize("name", ("all-2", "all-3", "all-8", "chain-8"))
def test_solve_byte_for_byte(eng, aref, name):
    """m = 2 with 1 edge, 3 with 3, 8 with 28 and 8 with a 7-edge chain, both weightings (INFO with matrices and mse of an alignment's size, and
    without matrices), apply 0 and 1: the record equals the host reference's byte for byte"""
    for seed in (0, 1):
        truths, ent, ed = A.exact_case(name, seed)
        rows = np.array(ed)
        rows["mse"] = np.random.default_rng(seed).uniform(0.2, 30.0, len(ed))
        for kw, infos in ((dict(weighting=UNIT), None), (dict(weighting=INFO), _infos(len(ed), seed)), (dict(weighting=INFO, apply=1, max_trials=3), None)):
            o = A.opts(aref, **kw)
            dev = eng.op_keyframe_adjust_solve(ent, rows, infos, **A.opts_kw(o))
            _same(dev, A.ref_solve(aref, ent, rows, o, infos)[0], (name, seed, kw))
            assert int(dev[0]["flags"]) & ADJUSTED and int(dev[0]["n_edges"]) == len(ed)
    # hostile rows and an entry that is not usable
    truths, ent, ed = A.exact_case(name, 2)
    e, rows = np.array(ent), np.array(ed)
    e[len(e) - 1]["h_origin_key"][0, 0] = np.nan
    rows["offsets_px"][0][2] = np.inf
    _same(eng.op_keyframe_adjust_solve(e, rows, None, weighting=UNIT), A.ref_solve(aref, e, rows, A.opts(aref, weighting=UNIT))[0], (name, "hostile"))
    _same(eng.op_keyframe_adjust_solve(ent, rows[:0], None), A.ref_solve(aref, ent, rows[:0], A.opts(aref))[0], (name, "no rows"))


@pytest.mark.parametrize("case", list(A.verdict_cases()))
def test_every_verdict_byte_for_byte(eng, aref, case):
    ent, ed, infos, kw, want = A.verdict_cases()[case]
    o = A.opts(aref, **kw)
    dev = eng.op_keyframe_adjust_solve(ent, ed, infos, **A.opts_kw(o))
    _same(dev, A.ref_solve(aref, ent, ed, o, infos)[0], case)
    assert int(dev[0]["flags"]) & A.VERDICTS == want


@pytest.fixture(scope="module")
def texture(eng, aref):
    """the whole call on the texture map with entry 1 displaced by 2 px -> (images, entries, options, device record, device level-0 records)"""
    images, exact, off = R.texture_map()
    o = A.opts(aref, **A.TEXTURE_OPTS)
    rec, er = eng.op_keyframe_adjust(images, off, want_edge_records=True, **A.opts_kw(o))
    return images, off, o, rec, er


def test_full_op_table_and_records(eng, aref, texture):
    """edges, jobs and starts equal the header's on the same entries; each edge's record equals hnet_op_photo_align_robust on the same two images and
    start, byte for byte; the whole record equals the host header run on the DEVICE's alignment records, byte for byte (7q's method: the host's own
    alignment sums in another order); without the records asked for the record is the same"""
    images, off, o, rec, er = texture
    r = rec[0]
    t = A.ref_pairs(aref, off, o.min_grid)[0]
    n = int(t["count"])
    assert (int(r["n_pairs"]), int(r["n_jobs"])) == (int(t["n_pairs"]), n) == (3, 3)
    for q in range(n):
        job = t["job"][q]
        for f in ("i", "j", "grid", "start_px"):
            assert r["edge"][q][f].tobytes() == job[f].tobytes(), (q, f)
        one = eng.op_photo_align_robust(images[int(job["i"])], images[int(job["j"])], job["start_px"], levels=o.levels, max_iterations=o.align.base.max_iterations)
        assert er[q].tobytes() == one[0].tobytes(), q
        assert r["edge"][q].tobytes()[:A.EDGE.itemsize - 16] == A.ref_judge(aref, job, er[q], o)[0].tobytes()[:A.EDGE.itemsize - 16], q
    assert er[n:].tobytes() == bytes(A.ROBUST.itemsize * (28 - n))
    _same(rec, A.ref_adjust_with(aref, off, er[:n], o)[0], "the header on the device's records")
    _same(eng.op_keyframe_adjust(images, off, **A.opts_kw(o)), rec, "without the edge records")
    # UNIT weights go through the same table
    ou = A.opts(aref, weighting=UNIT, **A.TEXTURE_OPTS)
    ru, eru = eng.op_keyframe_adjust(images, off, want_edge_records=True, **A.opts_kw(ou))
    assert eru.tobytes() == er.tobytes()
    _same(ru, A.ref_adjust_with(aref, off, er[:n], ou)[0], "UNIT weights")


def test_full_op_against_the_host_reference(aref, texture):
    """against the wholly-host reference (its own alignments): the integers are equal, delta_px differs by no more than 7q's margin of 1e-4 px"""
    images, off, o, rec, er = texture
    host, _, her = A.ref_adjust(aref, images, off, o)
    for f in ("flags", "anchor", "n_pairs", "n_jobs", "n_edges", "adjusted_mask", "unconnected_mask", "trials", "accepted", "pad"):
        assert int(rec[0][f]) == int(host[0][f]), f
    for f in ("i", "j", "grid", "flags"):
        assert rec[0]["edge"][f].tobytes() == host[0]["edge"][f].tobytes(), f
    d = float(np.abs(rec[0]["delta_px"] - host[0]["delta_px"]).max())
    print("worst |delta_px device - host| %.3e px; worst |offsets device - host| %.3e px" % (d, np.abs(er["px"]["offsets_px"] - her["px"]["offsets_px"]).max()))
    assert d <= A.HOST_DEVICE_GATE


def test_full_op_correction_and_render_after(eng, texture):
    """delta_px[1] is (-2, 0) on all four corners within twice the host reference's own deviation from that; rendering the adjusted entries in MEAN mode
    gives every entry an sse / n below the midpoint of 7ab's exact and displaced figures: more than half of the excess is gone"""
    images, off, o, rec, er = texture
    r = rec[0]
    assert int(r["flags"]) & ADJUSTED and int(r["anchor"]) == 0 and int(r["adjusted_mask"]) == 7
    dev = float(np.abs(r["delta_px"][1] - A.SHIFT_WANT).max())
    print("worst |delta_1 - (-2, 0)| %.4f px (gate %.4f)" % (dev, A.SHIFT_GATE))
    assert dev <= A.SHIFT_GATE
    adjusted = np.array(off)
    adjusted["h_origin_key"] = r["h_origin_key"][:3]
    got = R.seam_mse(eng.op_keyframe_render(images, adjusted, np.eye(3), 320, 224, _capi.RENDER_MEAN)[2])
    before = R.seam_mse(eng.op_keyframe_render(images, off, np.eye(3), 320, 224, _capi.RENDER_MEAN)[2])
    print("sse / n before", before, "after", got, "gates", A.RENDER_GATES)
    assert (got < np.array(A.RENDER_GATES)).all() and (before > np.array(A.RENDER_GATES)).all()


@pytest.mark.parametrize("seed", A.LOOP_SEEDS)
def test_drifted_loop(eng, seed):
    """six frames of one canvas on a closed path, steps of about 60 px, the entries the truth with 0.3 px of drift per link accumulated along the chain:
    the worst corner error against the truth starts at least three gates off and ends within the gate (twice the host reference's worst over the seeds,
    tests/test_keyframe_adjust_cpu.py::test_drifted_loop_reference_figures)"""
    images, truths, ent = A.drifted_loop(seed)
    rec = eng.op_keyframe_adjust(images, ent, **A.TEXTURE_OPTS)
    r = rec[0]
    before, after = A.worst_error(ent["h_origin_key"], truths), A.worst_error(r["h_origin_key"][:6], truths)
    print("seed", seed, "jobs", int(r["n_jobs"]), "edges", int(r["n_edges"]), "trials", int(r["trials"]), "worst corner error before %.4f after %.4f px" % (before, after))
    assert int(r["flags"]) & ADJUSTED and int(r["n_jobs"]) > 8 and int(r["adjusted_mask"]) == 63          # (more than one round)
    assert before >= A.LOOP_BEFORE_RATIO * A.LOOP_GATE and after <= A.LOOP_GATE


def test_four_rounds(eng, aref):
    """one map of 8 entries with 28 jobs is four rounds at max_batch 8: every row's record equals the alignment of its pair alone, whichever round it ran
    in, and the record equals the header on those records"""
    images, ent = R.pose_map(8)
    o = A.opts(aref, min_grid=1, min_overlap=0.3, **A.TEXTURE_OPTS)
    rec, er = eng.op_keyframe_adjust(images, ent, want_edge_records=True, **A.opts_kw(o))
    t = A.ref_pairs(aref, ent, 1)[0]
    assert int(rec[0]["n_jobs"]) == int(t["count"]) == 28
    for q in (0, 7, 8, 15, 16, 23, 24, 27):                                                                # the first and last row of every round
        job = t["job"][q]
        one = eng.op_photo_align_robust(images[int(job["i"])], images[int(job["j"])], job["start_px"], levels=o.levels, max_iterations=o.align.base.max_iterations)
        assert er[q].tobytes() == one[0].tobytes(), q
    _same(rec, A.ref_adjust_with(aref, ent, er, o)[0], "28 jobs")
    assert int(rec[0]["n_edges"]) >= 20
    again, er2 = eng.op_keyframe_adjust(images, ent, want_edge_records=True, **A.opts_kw(o))
    assert again.tobytes() == rec.tobytes() and er2.tobytes() == er.tobytes()


def test_op_refusals(eng):
    """every refusal of the two operator-level calls returns HNET_ERR_INVALID_ARG and writes nothing"""
    L = _capi.lib()
    images, exact, off = R.texture_map()
    truths, ent, ed = A.exact_case("all-3", 0)
    rec, er = np.full(A.REC.itemsize, 0xA5, np.uint8), np.full(28 * A.ROBUST.itemsize, 0xA5, np.uint8)
    p = lambda a: None if a is None else a.ctypes.data                         # noqa: E731

    def bad_opts():
        for k, v in (("levels", 0), ("levels", 5), ("min_grid", 0), ("min_grid", 65), ("min_overlap", 1.5), ("max_mse", -1.0), ("max_closure_px", np.nan),
                     ("weighting", 2), ("max_trials", 0), ("max_trials", 65), ("mse_floor", 0.0), ("lambda0", 0.0), ("lambda0", 1e101), ("eps_px", -1.0),
                     ("max_shift_px", np.inf), ("apply", 2), ("huber_k", -1.0), ("max_iterations", 33)):
            yield _capi.keyframe_adjust_opts(**{k: v})

    def solve(m=3, e=ent, n=3, rows=ed, o=_capi.keyframe_adjust_opts(), out=rec, ctx=eng.handle):
        return L.hnet_op_keyframe_adjust_solve(ctx, m, p(e), n, p(rows), None, C.addressof(o) if o is not None else None, p(out))

    def full(m=3, img=images, e=off, o=_capi.keyframe_adjust_opts(), out=rec, ctx=eng.handle):
        return L.hnet_op_keyframe_adjust(ctx, m, p(img), p(e), C.addressof(o) if o is not None else None, p(out), p(er) if out is not None else None)
    assert solve(ctx=None) == INVALID and full(ctx=None) == INVALID
    assert solve(m=0) == INVALID and solve(m=9) == INVALID and solve(n=-1) == INVALID and solve(n=29) == INVALID
    assert solve(e=None) == INVALID and solve(rows=None) == INVALID and solve(out=None) == INVALID and solve(o=None) == INVALID
    assert full(m=0) == INVALID and full(m=9) == INVALID and full(img=None) == INVALID and full(e=None) == INVALID and full(out=None) == INVALID
    assert full(o=None) == INVALID
    for o in bad_opts():
        assert solve(o=o) == INVALID and full(o=o) == INVALID
    assert (rec == 0xA5).all() and (er == 0xA5).all()
    assert solve() == 0 and not (rec == 0xA5).all() and solve(n=0, rows=None) == 0 and full() == 0             # what they were variations of is good
