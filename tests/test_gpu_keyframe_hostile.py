"""The keyframe layers on hostile steps on the device (include/hnet.h hnet_sessions_keyframe_track, _revisit, _relocalise, _relocalise_oriented;
csrc/kernels_keyframe.hip, kernels_keyframe_map.hip, kernels_photo_search.hip): the sequences of tests/keyframe_hostile.py, whose steps drive
the start, decide, note and select kernels into NO_START, a bridged lost frame, a restarted origin chain, an emptied map and a poisoned key_px.  Every
comparison is byte for byte; the file has no tolerance.  levels = 3 (4 for the relocalise), 6 trials; sessions objects of 4 cameras with a map of
capacity 3 on a context of max_batch 8.

As in tests/test_gpu_keyframe_map.py the host's state of a device session is the MIRROR: the functions of the shared headers run on the host
(tests/cpp/photo_search_oriented_ref.cpp and what it includes), fed the alignment records of the DEVICE.  After every call the device's record equals the
mirror's, its start_px the header's compose (or eight quiet NaNs), its rec hnet_op_photo_align_robust(the keyframe downloaded before the call, curr,
start_px), and map_info, every stored image and get_keyframe the mirror's.  The flag words are the constants of tests/keyframe_hostile.py, which
tests/test_keyframe_hostile_cpu.py checks against the host references: none is taken from the device."""
import numpy as np
import pytest

import keyframe_hostile as H
import keyframe_map_util as M
import keyframe_util as K
import photo_align_util as U
import photo_search_oriented_util as O
import photo_search_util as S
from cuahn_vio_amd import _capi

pytestmark = pytest.mark.gpu

N_CAM = 4
QNAN8 = np.full(8, H.QNAN, np.uint32).view(np.float32)


@pytest.fixture(scope="module")
def oref(tmp_path_factory):
    return O.build_ref(tmp_path_factory.mktemp("keyframe_hostile_ref_gpu"))


@pytest.fixture(scope="module")
def tab(oref):
    return np.ascontiguousarray(O.yaw_table(oref)[H.YAW13])


@pytest.fixture(scope="module")
def eng(blob):
    from cuahn_vio_amd.homography_net import HnetEngine
    e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=8)
    yield e
    e.close()


@pytest.fixture
def fleet(eng):
    from cuahn_vio_amd.homography_net import HnetSessions
    made = []

    def make():
        s = HnetSessions(eng, N_CAM)
        s.enable_keyframes()
        s.enable_keyframe_map(M.CAPACITY)
        made.append(s)
        return s
    yield make
    for s in made:
        s.close()


class Mirror(O.RefSession):
    """one device session restated on the host headers, from the device's alignment records"""

    def start(self, step):
        """the start the device has to compose for `step`: the header's compose, eight quiet NaNs where it fails, zeros without a keyframe"""
        if not self.state["has_key"][0]:
            return np.zeros(8, np.float32)
        start = K.ref_compose(self.lib, step, self.state["key_px"][0])
        return QNAN8.copy() if start is None else start

    def track(self, dev, frame, start, o):
        ns, want, copy = K.ref_decide(self.lib, self.state, start, dev["rec"], o)
        slot, self.mstate, self.entries = M.ref_note(self.lib, int(want["flags"][0]), copy, ns, self.mstate, self.entries)
        assert (slot >= 0) == bool(copy)
        self.state = ns
        if copy:
            self.key = np.array(frame, np.uint8)
            self.images[slot] = frame
        return want[0]

    def select(self, o):
        """-> (h_origin_before, slot, grid, start) as the revisit has to pick them"""
        ok, hb = M.ref_origin_curr(self.lib, self.state)
        if not ok:
            return hb, -1, 0, QNAN8.copy()
        return (hb,) + M.ref_select(self.lib, self.mstate, self.entries, hb, o.min_grid)

    def revisit(self, hb, slot, grid, start, rec, o):
        self.state, self.mstate, want, attach = M.ref_decide(self.lib, self.state, self.mstate, self.entries, slot, grid, start, hb, rec, o)
        if attach:
            self.key = self.images[slot].copy()
        return want[0]


def _snapshot(s, cam):
    """everything the keyframe layers hold of a session that the calls show: (entries, map state, images, keyframe)"""
    entries, mstate = s.keyframe_map_info(cam)
    return entries.tobytes(), mstate.tobytes(), np.stack([s.map_keyframe(cam, j) for j in range(M.CAPACITY)]).tobytes(), s.keyframe(cam).tobytes()


class Cam:
    """a camera of a device fleet and its mirror; every call is compared as the module's docstring says"""

    def __init__(self, eng, s, cam, lib, tab=None):
        self.eng, self.s, self.cam, self.mir, self.tab = eng, s, cam, Mirror(lib, M.CAPACITY), tab

    def same_state(self):
        return _snapshot(self.s, self.cam) == (self.mir.entries.tobytes(), self.mir.mstate.tobytes(), self.mir.images.tobytes(), self.mir.key.tobytes())

    def _align(self, template, frame, start, levels):
        return self.eng.op_photo_align_robust(template[None], frame[None], start[None], levels=levels, max_iterations=K.TRIALS)[0]

    def track(self, frame, step, o):
        had_key = bool(self.mir.state["has_key"][0])
        key = self.s.keyframe(self.cam) if had_key else None
        self.s.push([self.cam], frame[None])
        out = self.s.keyframe_track([self.cam], step[None], **K.opts_kw(o))[0]
        start = self.mir.start(step)
        assert out["start_px"].tobytes() == start.tobytes(), (out["start_px"], start)
        if had_key:
            assert key.tobytes() == self.mir.key.tobytes() and out["rec"].tobytes() == self._align(key, frame, start, o.levels).tobytes()
        else:
            assert not out["rec"].tobytes().strip(b"\0")
        want = self.mir.track(out, frame, start, o)
        assert out.tobytes() == want.tobytes(), (out["flags"], want["flags"])
        assert self.same_state()
        return out

    def revisit(self, frame, o):
        images = self.mir.images.copy()
        hb, slot, grid, start = self.mir.select(o)
        out = self.s.keyframe_revisit([self.cam], **M.opts_kw(o))[0]
        assert (int(out["slot"]), int(out["grid"])) == (slot, grid) and out["start_px"].tobytes() == start.tobytes()
        assert out["h_origin_before"].tobytes() == hb.tobytes()
        if slot >= 0:
            rec = self._align(images[slot], frame, start, o.levels)
            assert out["rec"].tobytes() == rec.tobytes()
        else:
            rec = np.zeros(1, K.REC)[0]
            assert not out["rec"].tobytes().strip(b"\0")
        want = self.mir.revisit(hb, slot, grid, start, rec, o)
        assert out.tobytes() == want.tobytes(), (out["flags"], want["flags"])
        assert self.same_state()
        return out

    def relocalise(self, kind, frame, o):
        key = self.s.keyframe(self.cam)
        if kind == "plain":
            out = self.s.keyframe_relocalise([self.cam], **S.reloc_kw(o))[0]
            want = self.mir.relocalise(frame, o, given=out["rv"]["rec"])
            search = self.eng.op_photo_search(key[None], frame[None], **S.search_kw(o.search))[0]
            start = out["search"]["start_px"]
        else:
            out = self.s.keyframe_relocalise_oriented([self.cam], hyps=self.tab, **S.reloc_kw(o))[0]
            want = self.mir.relocalise_oriented(frame, o, self.tab, given=out["rv"]["rec"])
            search = self.eng.op_photo_search_oriented(key[None], frame[None], hyps=self.tab, **S.search_kw(o.search))[0]
            start = out["search"]["base"]["start_px"]
        assert out.tobytes() == want.tobytes(), (out["rv"]["flags"], want["rv"]["flags"], out["target"], want["target"])
        assert int(out["target"]) == _capi.RL_TARGET_HELD and out["search"].tobytes() == search.tobytes()      # (the pinned records are the held keyframe's)
        assert out["rv"]["start_px"].tobytes() == start.tobytes() and out["rv"]["rec"].tobytes() == self._align(key, frame, start, o.levels).tobytes()
        assert self.same_state()
        return out


@pytest.mark.parametrize("seed,name,auto_rekey", H.TRACK_CASES)
def test_track(eng, fleet, oref, seed, name, auto_rekey):
    """(a): frames 0 .. 4 with the hostile step at frame 2, every call compared by Cam.track; the five flag words are the host reference's"""
    cam = Cam(eng, fleet(), 1, oref)
    recs = H.run_track(seed, name, auto_rekey, cam.track)
    assert tuple(int(r["flags"]) for r in recs) == H.track_flags(seed, name, auto_rekey)
    hostile = recs[H.TRACK_AT]
    if name in H.NO_COMPOSE:                                                 # the quiet-NaN start, a DEGENERATE record, the previous key_px as the bridge
        assert (hostile["start_px"].view(np.uint32) == H.QNAN).all() and hostile["rec"]["px"]["flags"] & U.DEGENERATE
        assert hostile["key_px"].tobytes() == recs[H.TRACK_AT - 1]["key_px"].tobytes()
    else:                                                                    # a finite start far outside the image, which is also the bridge
        assert np.isfinite(hostile["start_px"]).all() and np.abs(hostile["start_px"]).min() > 0.99 * float(name)
        assert hostile["key_px"].tobytes() == hostile["start_px"].tobytes()
    assert all(np.isfinite(r["h_origin_curr"]).all() for r in recs)
    for other in (0, 2, 3):                                                  # the sessions no call listed hold nothing
        entries, mstate = cam.s.keyframe_map_info(other)
        assert not entries.view(np.uint8).any() and not mstate.view(np.uint8).any()


@pytest.mark.parametrize("seed,name,auto_rekey", H.MAP_CASES)
def test_map(eng, fleet, oref, seed, name, auto_rekey):
    """(b): the hostile step at frame 4 of a session with a map, a revisit on it, frame 5, a revisit on it, every call compared by Cam.track and
    Cam.revisit; the flag words, the revisits' (flags, slot, links, grid) and the map's validity and state words are the host reference's"""
    cam = Cam(eng, fleet(), 2, oref)
    want, snaps = H.MAP_EXPECT[name, auto_rekey], []

    def after(i):
        if H.map_snapshots(i) is not None:
            entries, mstate = cam.s.keyframe_map_info(cam.cam)
            snaps.append((tuple(entries["valid"].tolist()), tuple(int(mstate[f][0]) for f in ("cur_slot", "cur_links", "cursor", "serial"))))
    recs, rvs = H.run_map(seed, name, auto_rekey, cam.track, cam.revisit, after)
    assert tuple(int(r["flags"]) for r in recs) == H.map_flags(seed, name, auto_rekey)
    assert tuple((int(r["flags"]), int(r["slot"]), int(r["links"]), int(r["grid"])) for r in rvs) == want["rv"]
    assert tuple(s[0] for s in snaps) == want["valid"] and tuple(s[1] for s in snaps) == want["mstate"], snaps
    assert all(np.isfinite(r["h_origin_curr"]).all() for r in recs + rvs)


@pytest.mark.parametrize("seed,kind", H.RELOC_CASES)
def test_relocalise_from_a_poisoned_session(eng, fleet, oref, tab, seed, kind):
    """(c): the session whose key_px a 1e12 step left far outside the image is RETRACKED on its held keyframe by the plain and by the oriented
    relocalise, as on the host; the search record is hnet_op_photo_search's (_oriented's) and the level-0 record hnet_op_photo_align_robust's from the
    searched start; the next track with the true step is an ordinary tracked frame"""
    cam = Cam(eng, fleet(), 3, oref, tab)
    recs, rl, nxt = H.run_reloc(seed, cam.track, lambda frame, o: cam.relocalise(kind, frame, o))
    assert tuple(int(r["flags"]) for r in recs) == H.RELOC_TRACKS[seed]
    assert np.abs(recs[-1]["key_px"]).min() > 0.99e12
    assert (int(rl["rv"]["flags"]), int(rl["target"]), int(rl["n_searched"]), int(rl["n_found"])) == H.RELOC_ANSWER
    assert int(nxt["flags"]) == H.RELOC_NEXT and int(nxt["age"]) == H.RELOC_AT + 1 and int(nxt["keyframes"]) == 1
    assert cam.s.keyframe(cam.cam).tobytes() == K.sequence("out-and-back", seed)[0][0].tobytes()


# the crowd: session -> (the seed of its sequence, its step at frame 2)
CROWD = {2: (5, "nan"), 0: (5, "1e13"), 3: (2, "1e12"), 1: (2, None)}
CROWD_ORDER = [2, 0, 3, 1]


@pytest.mark.parametrize("auto_rekey", [1, 0])
def test_crowd(fleet, auto_rekey):
    """one call of n = 4, ids out of order, holds a NaN step, the 1e13 step, the 1e12 step and a benign one.  Each session's record and everything it
    holds afterwards equal those of the same session tracked alone on a second fleet, where a call that lists one session leaves the three others as
    they are; so does the next call (frame 3, true steps), which shows the states.  The flag words are the host reference's"""
    a, b = fleet(), fleet()
    kw = K.opts_kw(H.track_opts(auto_rekey))
    seqs = {c: (K.sequence("out-and-back", seed)[0], K.sequence("out-and-back", seed)[2] if name is None else H.hostile_steps(seed, name, H.TRACK_AT))
            for c, (seed, name) in CROWD.items()}

    def call(s, ids, i):
        s.push(ids, np.stack([seqs[c][0][i] for c in ids]))
        return s.keyframe_track(ids, np.stack([seqs[c][1][i] for c in ids]), **kw)
    for i in range(H.TRACK_AT):
        assert call(a, CROWD_ORDER, i).tobytes() == call(b, CROWD_ORDER, i).tobytes()
    for i in (H.TRACK_AT, H.TRACK_AT + 1):
        alone = {}
        for c in CROWD_ORDER:
            keep = {x: _snapshot(b, x) for x in range(N_CAM) if x != c}
            alone[c] = call(b, [c], i)[0]
            assert keep == {x: _snapshot(b, x) for x in range(N_CAM) if x != c}, (i, c)
        out = call(a, CROWD_ORDER, i)
        for j, c in enumerate(CROWD_ORDER):
            seed, name = CROWD[c]
            assert out[j].tobytes() == alone[c].tobytes(), (i, c, out[j]["flags"], alone[c]["flags"])
            assert _snapshot(a, c) == _snapshot(b, c), (i, c)
            assert int(out[j]["flags"]) == (0 if name is None else H.track_flags(seed, name, auto_rekey)[i]), (i, c)


def test_stuck_session(eng, fleet, oref):
    """auto_rekey = 0 after the 1e13 step: three further frames each answer NO_START | ORIGIN_RESTARTED with the same key_px, h_origin_curr = I and
    everything the session holds byte-identical (Cam.track compares the state with the mirror's, whose age alone counts on); after
    hnet_sessions_keyframe_reset the next track is FIRST"""
    cam = Cam(eng, fleet(), 0, oref)
    snaps = []

    def track(frame, step, o):
        out = cam.track(frame, step, o)
        snaps.append((_snapshot(cam.s, cam.cam), cam.mir.state.copy()))
        return out
    recs, further = H.run_stuck(track)
    assert tuple(int(r["flags"]) for r in recs) == H.track_flags(H.STUCK_SEED, H.STUCK_STEP, 0)
    assert tuple(int(r["flags"]) for r in further) == H.STUCK_FLAGS
    snap0, st0 = snaps[H.TRACK_FRAMES - 1]
    for k, (r, (snap, st)) in enumerate(zip(further, snaps[H.TRACK_FRAMES:])):
        assert snap == snap0 and st["key_px"].tobytes() == st0["key_px"].tobytes() and st["h_origin_key"].tobytes() == st0["h_origin_key"].tobytes()
        assert int(r["age"]) == H.STUCK_FURTHER[k] and r["key_px"].tobytes() == st0["key_px"][0].tobytes() and r["h_origin_curr"].tobytes() == np.eye(3).tobytes()
    cam.s.keyframe_reset(cam.cam)
    cam.mir.reset()
    frames, _, steps = K.sequence("out-and-back", H.STUCK_SEED)
    cam.s.push([cam.cam], frames[8:9])
    out = cam.s.keyframe_track([cam.cam], steps[8:9], **K.opts_kw(H.track_opts(0)))[0]
    assert int(out["flags"]) == H.FIRST and int(out["keyframes"]) == 1 and cam.s.keyframe(cam.cam).tobytes() == frames[8].tobytes()
    entries, mstate = cam.s.keyframe_map_info(cam.cam)
    assert entries["valid"].tolist() == [1, 0, 0] and tuple(int(mstate[f][0]) for f in ("cur_slot", "cur_links", "cursor", "serial")) == (0, 0, 0, 1)
