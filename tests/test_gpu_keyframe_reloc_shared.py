"""The three relocalising calls on ONE store (include/hnet.h hnet_sessions_keyframe_relocalise, hnet_sessions_keyframe_relocalise_oriented,
hnet_sessions_keyframe_track_recover): they share one scratch, so whatever one of them leaves there must not show in another, and a full batch
must not run one session's sections into its neighbour's.  A context of max_batch 2 and sessions objects of 2 cameras, without a map (capacity 0) and
with the largest one (8 slots, all filled), under the default table of 60 entries and under one of 64: the extreme sizes of every section of the scratch.
Every comparison is byte for byte; what the calls compute is tests/test_gpu_keyframe_reloc*.py's and tests/test_gpu_keyframe_recover.py's subject.

The frames: per camera a path of 16 distinct views on photo_search_util's wide canvas, 3.6 px further from the keyframe's view and a fresh draw of 0.5 px
corner offsets per frame (no view repeats, so no candidate is ever the current frame itself), and a far view (photo_search_util.VIEWS[0], 96 px from the
keyframe's view on the other side, within the search radius of every frame of the path) that a track with max_mse = 120 calls LOST."""
import functools

import numpy as np
import pytest

import keyframe_recover_util as KR
import keyframe_util as K
import photo_search_oriented_util as O
import photo_search_util as S
from cuahn_vio_amd import _capi, synth

pytestmark = pytest.mark.gpu

N_CAM = 2
IDS = [1, 0]                                    # the full batch, out of order
SEEDS = (2, 5)                                  # camera 0's and camera 1's canvas
PATH = 16
CAPACITIES = (0, _capi.KEYFRAME_MAP_MAX_CAPACITY)
TABLES = (60, 64)
KINDS = ("plain", "oriented", "recover")
assert O.ORELOC.itemsize == S.RELOC.itemsize + 64 and KR.RECOVER.itemsize == K.TRACK.itemsize + O.ORELOC.itemsize


@functools.lru_cache(maxsize=None)
def path(seed):
    """-> (frames u8 [PATH, 224, 320], true steps f32 [PATH, 8] (row i: frame i - 1 -> i; row 0 zero), the far frame): nobody modifies them"""
    cv = S.wide_canvas(seed)
    poses = [np.tile(np.array([3.0 * k, -2.0 * k]), 4) + synth.true_offsets(seed + 700 + k, 0.5) for k in range(PATH)]
    frames = np.stack([S.render_wide(cv, p) for p in poses])
    steps = np.zeros((PATH, 8), np.float32)
    for i in range(1, PATH):
        steps[i] = K.relative(poses[i - 1], poses[i]).astype(np.float32)
    return frames, steps, S.render_wide(cv, S.view_pose(seed, 0))


def table(entries):
    return _capi.photo_search_yaw_table() if entries == 60 else _capi.photo_search_yaw_table(-96.0, 3.0, 64)


def batch(t, far=()):
    """frame t of each listed camera's path and its step; the cameras in `far` see their far frame from a zero step instead"""
    frames = np.stack([path(SEEDS[c])[2] if c in far else path(SEEDS[c])[0][t] for c in IDS])
    steps = np.stack([np.zeros(8, np.float32) if c in far else path(SEEDS[c])[1][t] for c in IDS])
    return frames, steps


@pytest.fixture(scope="module")
def eng(blob):
    from cuahn_vio_amd.homography_net import HnetEngine
    e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=N_CAM)
    yield e
    e.close()


@pytest.fixture
def fleet(eng):
    from cuahn_vio_amd.homography_net import HnetSessions
    made = []

    def make(capacity):
        s = HnetSessions(eng, N_CAM)
        s.enable_keyframes()
        if capacity:
            s.enable_keyframe_map(capacity)
        made.append(s)
        return s
    yield make
    for s in made:
        s.close()


def store(s, capacity):
    """every byte the keyframe layers hold: per camera the keyframe, and with a map the entries, the map state and the images"""
    out = []
    for cam in range(N_CAM):
        out.append(s.keyframe(cam).tobytes())
        if capacity:
            entries, mstate = s.keyframe_map_info(cam)
            out += [entries.tobytes(), mstate.tobytes()] + [s.map_keyframe(cam, i).tobytes() for i in range(capacity)]
    return tuple(out)


def fill(s, capacity):
    """frames 0 .. capacity tracked with max_age = 1 (every slot of the map holds a keyframe), one more with auto_rekey = 0 (the held keyframe is not the
    current frame) -> the next frame's index"""
    ticks = max(capacity, 1) + 1
    for t in range(ticks + 1):
        frames, steps = batch(t)
        s.push(IDS, frames)
        s.keyframe_track(IDS, steps if t else None, **K.opts_kw(K.opts(levels=S.LEVELS, max_age=1) if t < ticks else TRACK))
    if capacity:
        for cam in range(N_CAM):
            assert s.keyframe_map_info(cam)[0]["valid"].all()
    return ticks + 1


TRACK = K.opts(levels=S.LEVELS, auto_rekey=0, max_mse=KR.MAX_MSE)     # after the fill: the keyframe stays, a far frame is LOST
# max_closure_px = 1e-6: every candidate is searched, the alignment runs against the pick and the call is REJECTED (tools/photo_search_bench.py), so an
# object on which a relocalising call is left out holds the state of one on which it was made
REJECT = S.reloc_opts(max_closure_px=1e-6)


def call(s, kind, ids, steps, tab, reloc):
    if kind == "plain":
        return s.keyframe_relocalise(ids, **S.reloc_kw(reloc))
    if kind == "oriented":
        return s.keyframe_relocalise_oriented(ids, hyps=tab, **S.reloc_kw(reloc))
    return s.keyframe_track_recover(ids, steps, hyps=tab, track=TRACK, reloc=reloc)


def run(s, capacity, tab, order, only=None):
    """per kind of `order` one tick: the next frames pushed and tracked (by the recovering call itself in its tick, where camera `tick % 2` sees its far
    frame), then the kind's call when `only` is None or the kind -> the records of the calls made and the store after every tick"""
    t = fill(s, capacity)
    recs, stores = [], []
    for tick, kind in enumerate(order):
        frames, steps = batch(t + tick, far=(tick % 2,) if kind == "recover" else ())
        s.push(IDS, frames)
        mine = only in (None, kind)
        if kind != "recover" or not mine:
            s.keyframe_track(IDS, steps, **K.opts_kw(TRACK))
        if mine:
            out = call(s, kind, IDS, steps, tab, REJECT)
            rv = out["reloc"]["rv"] if kind == "recover" else out["rv"]
            assert not (rv["flags"] & (_capi.RL_ATTACHED | _capi.RL_RETRACKED)).any()
            if kind == "recover":
                lost = (out["track"]["flags"] & _capi.KF_LOST) != 0
                assert lost[IDS.index(tick % 2)] and (out["reloc"]["n_searched"][lost] == (capacity or 1)).all()
            else:
                assert (out["n_searched"] == (capacity or 1)).all() and (out["n_found"] >= 1).all()
            recs.append((kind, out.tobytes()))
        stores.append(store(s, capacity))
    return recs, stores


@pytest.mark.parametrize("order", [KINDS + KINDS, KINDS[::-1] + KINDS[::-1]], ids=["plain-first", "recover-first"])
@pytest.mark.parametrize("entries", TABLES)
@pytest.mark.parametrize("capacity", CAPACITIES)
def test_interleaved_on_one_store(fleet, capacity, entries, order):
    """the three calls in turn on one object, twice over, against twin objects on which one kind is the only relocalising call ever made: the records of
    each kind and the stores after every tick are equal"""
    tab = table(entries)
    recs, stores = run(fleet(capacity), capacity, tab, order)
    assert [k for k, _ in recs] == list(order)
    for kind in KINDS:
        twin_recs, twin_stores = run(fleet(capacity), capacity, tab, order, only=kind)
        assert twin_recs == [r for r in recs if r[0] == kind], kind
        assert twin_stores == stores, kind


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("entries", TABLES)
@pytest.mark.parametrize("capacity", CAPACITIES)
def test_full_batch_against_singles(fleet, capacity, entries, kind):
    """one call of the full batch against the same two sessions called one at a time on a twin, under the default options (the sessions are re-tracked,
    re-attached or recovered where the call finds them): the records and the stores are equal.  Both cameras see their far frame in the recovering call."""
    tab, reloc = table(entries), S.reloc_opts()
    a, b = fleet(capacity), fleet(capacity)
    t = fill(a, capacity)
    assert fill(b, capacity) == t
    frames, steps = batch(t, far=IDS if kind == "recover" else ())
    for s in (a, b):
        s.push(IDS, frames)
        if kind != "recover":
            s.keyframe_track(IDS, steps, **K.opts_kw(TRACK))
    full = call(a, kind, IDS, steps, tab, reloc)
    singles = [call(b, kind, [cam], steps[i:i + 1], tab, reloc)[0] for i, cam in enumerate(IDS)]
    assert [r.tobytes() for r in full] == [r.tobytes() for r in singles]
    assert store(a, capacity) == store(b, capacity)
    if kind == "recover":
        assert ((full["track"]["flags"] & _capi.KF_LOST) != 0).all()
        full = full["reloc"]
    assert (full["n_searched"] == (capacity or 1)).all()
