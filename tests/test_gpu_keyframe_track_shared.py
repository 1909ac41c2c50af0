"""In-step keyframe tracks and sessions-level keyframe calls on ONE store (include/hnet.h hnet_filters_set_keyframe_measure, hnet_filters_set_keyframe_recover,
hnet_sessions_keyframe_relocalise, hnet_sessions_keyframe_relocalise_oriented, hnet_sessions_keyframe_revisit): the track of a filter step
and the sessions calls share one launch sequence and the store's scratch blocks, so whatever a sessions call leaves there must not show in the next
step's track, and an in-step track at a full batch must not run one session's sections into its neighbour's.  A context of max_batch 2 and sessions
objects of 2 cameras stepped as [1, 0], 1 IEKF iteration, without a map (capacity 0) and with the largest one (8 slots), the recover table as the identity
entry alone and as 64 entries.  Every comparison is byte for byte; what the calls compute is tests/test_gpu_filters_keyframe*.py's and
tests/test_gpu_keyframe*.py's subject.

The paths, seven ticks, both cameras measuring and recovering under the kidnapped_map row's options (max_age = 1: every tracked frame is a new
keyframe and, with a map, a new entry).  Camera 0 walks the kidnapped_map row of seed 5 (keyframe_recover_util.row): four tracked frames, the constant
frame (lost, unrecovered), the far frame on tick 5 (with a map: re-attached to a stored keyframe), the frame after it.  Camera 1 walks the kidnapped row
of seed 2: its keyframe's view, the kidnapped frame on tick 1 (re-tracked on its held keyframe, the measurement taken from the relocalise's record), the
row's next frame, and four more on the row's canvas, each a fresh draw of 2 px corner offsets from the one before, tracked from its true step.  No
frame repeats: a stored keyframe that IS the current frame would align with a closure of exactly 0, which no max_closure_px rejects.  On the host
reference alone (filters_keyframe_recover_util.RefFilterSession at capacity 8 and 0, both tables) these paths give per tick the measure flags
  camera 0: FIRST, APPLIED x 3, TRACK_LOST, REATTACHED with RL_ATTACHED (capacity 0: TRACK_LOST, then TRACK_GAP), APPLIED
  camera 1: FIRST, APPLIED | FROM_RELOC with RL_RETRACKED, APPLIED x 5
so the records compared below are not empty ones; the device's own flags are asserted at the end."""
import functools

import numpy as np
import pytest

import filters_keyframe_recover_util as FR
import filters_keyframe_util as FK
import keyframe_recover_util as KR
import keyframe_util as K
import photo_search_util as S
import test_gpu_filters as tg
import test_gpu_filters_keyframe as gk
import test_gpu_filters_photo_gate as pg
from cuahn_vio_amd import synth
from test_gpu_filters_photo_gate import _close_in_order  # noqa: F401  (autouse: closes what pg._track holds, the last one first)

pytestmark = pytest.mark.gpu

N_CAM = 2
IDS = np.array([1, 0], np.int32)                # the full batch, out of order
ROW = "kidnapped_map"                           # whose measure and reloc options serve both cameras
SEEDS = (5, 2)                                  # camera 0's kidnapped_map row, camera 1's kidnapped row
TICKS = 7
KIDNAPPED = {1: 1, 5: 0}                        # tick -> the camera that is kidnapped on it
CAPACITIES = (0, 8)
TABLES = (1, 64)
# max_closure_px = 1e-6: the call searches, aligns and is REJECTED (tests/test_gpu_keyframe_reloc_shared.py REJECT), so it leaves the store as it was
REJECT = S.reloc_opts(max_closure_px=1e-6)


def table(entries):
    _capi = tg._mods()[0]
    return _capi.photo_search_yaw_table(0.0, 1.0, 1) if entries == 1 else _capi.photo_search_yaw_table(-180.0, 5.625, 64)


@functools.lru_cache(maxsize=None)
def paths():
    """-> per camera (frames [TICKS], steps [TICKS] f32 [8]): nobody modifies them"""
    km, kd = KR.row(ROW, SEEDS[0]), KR.row("kidnapped", SEEDS[1])
    zero = np.zeros(8, np.float32)
    cv, poses = S.wide_canvas(SEEDS[1]), [S.kidnapped(SEEDS[1])[1][2]]
    for k in range(TICKS - 3):
        poses.append(poses[-1] + synth.true_offsets(SEEDS[1] + 801 + k, 2.0))
    frames1 = list(kd["frames"]) + [S.render_wide(cv, q) for q in poses[1:]]
    steps1 = [zero, zero, FR.row_step(kd, 2)] + [K.relative(poses[k], poses[k + 1]).astype(np.float32) for k in range(TICKS - 3)]
    assert len({fr.tobytes() for fr in list(km["frames"]) + frames1}) == 2 * TICKS
    return (list(km["frames"]), [FR.row_step(km, i) for i in range(TICKS)]), (frames1, steps1)


def rig(blob, capacity, tab):
    """a filters object on 2 cameras and a context of max_batch 2: keyframes (and a map), measure and recovery on for both cameras, a network that
    applies nothing (k_net_cov = 1e12, as the rows of tests/test_gpu_filters_keyframe_recover.py)"""
    HnetFilters = tg._mods()[3]
    e, s, f = pg._track(*tg._setup(blob, N_CAM, 1, max_batch=N_CAM))
    f.enable_innovations()
    s.enable_keyframes()
    if capacity:
        s.enable_keyframe_map(capacity)
    rng = np.random.default_rng(3)
    for i in range(N_CAM):
        p = tg._params(HnetFilters, rng, i)
        p.k_net_cov = 1e12
        f.set_params(i, p)
        f.set_keyframe_measure(i, FR.row_measure_opts(ROW))
        f.set_keyframe_recover(i, KR.reloc_opts(ROW), hyps=tab)
    return e, s, f


def store(s, capacity):
    """every byte the keyframe layers hold: per camera the keyframe, and with a map the entries, the map state and the images"""
    out = []
    for cam in range(N_CAM):
        out.append(s.keyframe(cam).tobytes())
        if capacity:
            entries, mstate = s.keyframe_map_info(cam)
            out += [entries.tobytes(), mstate.tobytes()] + [s.map_keyframe(cam, i).tobytes() for i in range(capacity)]
    return out


def tick(s, f, ids, t):
    """tick t of the listed cameras' paths -> per listed camera (measure | relocalise record, state, outputs, update count)"""
    pa = paths()
    time = gk.T0 + 0.1 * t
    out, net, upd = gk._tick(s, f, ids, [pa[c][0][t] for c in ids], time, [FK.row_state(pa[c][1][t], time - 0.05) for c in ids])
    rr, st = f.last_keyframe_recover(len(ids)), f.get_state(ids)
    return {int(c): (rr[k].tobytes(), st[k].tobytes(), out[k].tobytes(), net[:, k].tobytes(), int(upd[k])) for k, c in enumerate(ids)}, rr


def rejected_calls(s, capacity, tab):
    """the three sessions-level calls that share the track's scratch, each REJECTED on both cameras"""
    _capi = tg._mods()[0]
    kw = S.reloc_kw(REJECT)
    a, b = s.keyframe_relocalise(IDS, **kw), s.keyframe_relocalise_oriented(IDS, hyps=tab, **kw)
    for rv in (a["rv"], b["rv"]):
        assert not (rv["flags"] & (_capi.RL_ATTACHED | _capi.RL_RETRACKED)).any()
    if capacity:
        rv = s.keyframe_revisit(IDS, levels=K.LEVELS, max_iterations=S.TRIALS, max_closure_px=1e-6)
        assert not (rv["flags"] & _capi.RV_ATTACHED).any()


@pytest.mark.parametrize("entries", TABLES)
@pytest.mark.parametrize("capacity", CAPACITIES)
def test_instep_tracks_among_sessions_calls(blob, capacity, entries):
    """(a) fleet A makes hnet_sessions_keyframe_relocalise, _relocalise_oriented and, with a map, _revisit on its sessions object between every two
    ticks, each REJECTED; its twin B never does: the measure and relocalise records of every tick, the filter states, outputs and update counts and every
    byte of the store are equal.  (b) a third fleet C steps the two kidnapped ticks as [1] then [0] where A steps [1, 0]: the same.  Over the ticks a
    slot has FROM_RELOC, a slot has APPLIED and, with a map, a slot is REATTACHED."""
    _capi = tg._mods()[0]
    tab = table(entries)
    (ea, sa, fa), (eb, sb, fb), (ec, sc, fc) = (rig(blob, capacity, tab) for _ in range(3))
    flags, rflags = 0, 0
    for t in range(TICKS):
        a, rr = tick(sa, fa, IDS, t)
        b, _ = tick(sb, fb, IDS, t)
        if t in KIDNAPPED:
            c = {}
            for cam in IDS:
                c.update(tick(sc, fc, np.array([cam], np.int32), t)[0])
            assert rr["m"]["track"]["flags"][list(IDS).index(KIDNAPPED[t])] & _capi.KF_LOST, t
        else:
            c, _ = tick(sc, fc, IDS, t)
        print(f"capacity {capacity}, {entries} entries, tick {t}: flags {[hex(int(x)) for x in rr['m']['flags']]}, track {[hex(int(x)) for x in rr['m']['track']['flags']]}, "
              f"reloc {[hex(int(x)) for x in rr['reloc']['rv']['flags']]}")
        assert a == b, t
        assert a == c, t
        assert store(sa, capacity) == store(sb, capacity) == store(sc, capacity), t
        flags |= int(np.bitwise_or.reduce(rr["m"]["flags"]))
        rflags |= int(np.bitwise_or.reduce(rr["reloc"]["rv"]["flags"]))
        rejected_calls(sa, capacity, tab)
        assert store(sa, capacity) == store(sb, capacity), t
    assert flags & FR.FROM_RELOC and flags & FK.APPLIED
    assert not capacity or flags & FR.REATTACHED or rflags & _capi.RL_ATTACHED
    for o in (fa, fb, fc, sa, sb, sc, ea, eb, ec):
        o.close()
