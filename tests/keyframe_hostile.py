"""What the CPU and the GPU tests of the keyframe layers on hostile steps share (include/hnet_keyframe.h, include/hnet_keyframe_map.h,
include/hnet_keyframe_reloc.h): the named hostile steps, the three kinds of sequence built on keyframe_util.sequence("out-and-back", seed) for
seeds 2 and 5, and the flag word of every record as the host references (tests/cpp/keyframe_ref.cpp, keyframe_map_ref.cpp, photo_search_ref.cpp,
photo_search_oriented_ref.cpp) gave it.  tests/test_keyframe_hostile_cpu.py checks every constant against those references; the GPU file asserts them of
the device.  Nothing here is taken from the device."""
import numpy as np

import keyframe_map_util as M
import keyframe_util as K
import photo_search_util as S
from cuahn_vio_amd import _capi

SEEDS = (2, 5)
QNAN = 0x7FC00000                          # the bits of every entry of a start that could not be composed


def _all(v):
    return np.full(8, v, np.float32)


def _one(k, v):
    o = np.zeros(8, np.float32)
    o[k] = v
    return o


# The hostile steps (prev -> curr offsets, f32 [8]).  The first six cannot be composed (NO_START); the rest compose to a finite start far outside the
# image, on which the alignment stops.  1e12 puts |m[8]| of the origin chain's product on the boundary of chain()'s 1e-12 test, 1e13 beyond it.
STEPS = {
    "nan": _all(np.nan),
    "nan3": _one(3, np.nan),
    "inf": _all(np.inf),
    "3e38": _all(3e38),
    "1e30": _all(1e30),
    "bowtie": np.array([0, 0, 0, 0, -319, -223, 0, 0], np.float32),      # br onto ul: a corner's z is not positive
    "1e13": _all(1e13),
    "1e12": _all(1e12),
    "1e6": _all(1e6),
}
NO_COMPOSE = ("nan", "nan3", "inf", "3e38", "1e30", "bowtie")
FINITE_FAR = ("1e13", "1e12", "1e6")

FIRST = _capi.KF_FIRST | _capi.KF_REKEYED
NO_START, STOPPED, BRIDGED, REKEYED, RESTARTED = _capi.KF_NO_START, _capi.KF_STOPPED, _capi.KF_BRIDGED, _capi.KF_REKEYED, _capi.KF_ORIGIN_RESTARTED
EVERY = _capi.KF_REKEYED | _capi.KF_MAX_AGE                             # a tracked frame under max_age = 1
NO_CANDIDATE, ATTACHED, RETRACKED = _capi.RV_NO_CANDIDATE, _capi.RV_ATTACHED, _capi.RL_RETRACKED

# ---- (a) track: frames 0 .. 4, default options but auto_rekey, the hostile step at frame 2
TRACK_AT, TRACK_FRAMES = 2, 5
# (step, auto_rekey) -> the flags of the five records, where both seeds give the same
TRACK_FLAGS = {}
for _n in NO_COMPOSE:
    TRACK_FLAGS[_n, 1] = (FIRST, 0, NO_START | BRIDGED | REKEYED, 0, 0)
    TRACK_FLAGS[_n, 0] = (FIRST, 0, NO_START, 0, 0)
TRACK_FLAGS["1e13", 1] = (FIRST, 0, STOPPED | BRIDGED | REKEYED | RESTARTED, 0, 0)
TRACK_FLAGS["1e12", 1] = (FIRST, 0, STOPPED | BRIDGED | REKEYED, 0, 0)
TRACK_FLAGS["1e6", 1] = (FIRST, 0, STOPPED | BRIDGED | REKEYED, 0, 0)
# (step, seed) -> the same without a re-key.  The session keeps the far key_px, and what the next frames answer depends on the seed: composing the true
# step with a key_px of 1e6 .. 1e13 gives four corners of positive z (a finite start far outside the image, on which the alignment stops: STOPPED, and
# BRIDGED where H(start) is finite) or not (NO_START).  Seed 5 is the sequence of the table in DESIGN 7t.
TRACK_FLAGS_STUCK = {
    ("1e13", 2): (FIRST, 0, STOPPED | BRIDGED | RESTARTED, STOPPED | RESTARTED, STOPPED | RESTARTED),
    ("1e13", 5): (FIRST, 0, STOPPED | BRIDGED | RESTARTED, NO_START | RESTARTED, NO_START | RESTARTED),
    ("1e12", 2): (FIRST, 0, STOPPED | BRIDGED, STOPPED, STOPPED),
    ("1e12", 5): (FIRST, 0, STOPPED | BRIDGED, NO_START, NO_START),
    ("1e6", 2): (FIRST, 0, STOPPED | BRIDGED, STOPPED | BRIDGED, STOPPED | BRIDGED),
    ("1e6", 5): (FIRST, 0, STOPPED | BRIDGED, NO_START, NO_START),
}
TRACK_CASES = [(seed, name, ar) for seed in SEEDS for name in STEPS for ar in (1, 0)]


# The stuck session: seed 2, the 1e13 step, auto_rekey = 0, run on through frames 5, 6 and 7 with their true steps.  Each of the three answers
# NO_START | ORIGIN_RESTARTED and leaves key_px, h_origin_key, the keyframe and the (empty) map as they were; only the age counts on.
STUCK_SEED, STUCK_STEP, STUCK_FURTHER = 2, "1e13", (5, 6, 7)
STUCK_FLAGS = (NO_START | RESTARTED,) * 3


def track_flags(seed, name, auto_rekey):
    """the flags of the five records of (a)"""
    return TRACK_FLAGS[name, auto_rekey] if (name, auto_rekey) in TRACK_FLAGS else TRACK_FLAGS_STUCK[name, seed]


def track_opts(auto_rekey):
    return K.opts(auto_rekey=auto_rekey)


def hostile_steps(seed, name, at):
    """the steps of the sequence with the hostile one in place of frame `at`'s"""
    steps = K.sequence("out-and-back", seed)[2].copy()
    steps[at] = STEPS[name]
    return steps


def run_track(seed, name, auto_rekey, track):
    """(a) on any session: track(frame, step, opts) -> TRACK record; -> the five records"""
    frames, steps, o = K.sequence("out-and-back", seed)[0], hostile_steps(seed, name, TRACK_AT), track_opts(auto_rekey)
    return [track(frames[i], steps[i], o) for i in range(TRACK_FRAMES)]


def run_stuck(track):
    """the stuck session on any session -> (the five records of (a), the three further ones)"""
    frames, steps, o = K.sequence("out-and-back", STUCK_SEED)[0], hostile_steps(STUCK_SEED, STUCK_STEP, TRACK_AT), track_opts(0)
    return [track(frames[i], steps[i], o) for i in range(TRACK_FRAMES)], [track(frames[i], steps[i], o) for i in STUCK_FURTHER]


# ---- (b) map: capacity 3, max_age = 1 with auto_rekey (a re-key at every frame) and 0 without (the keyframe stays frame 0), frames 0 .. 4 with the
# hostile step at frame 4, a revisit on frame 4, a track of frame 5 with its true step, a revisit on frame 5: eight calls
MAP_AT, MAP_STEPS, MAP_CALLS = 4, ("1e13", "1e12", "1e6", "nan"), 8
MAP_CASES = [(seed, name, ar) for seed in SEEDS for name in MAP_STEPS for ar in (1, 0)]
_ALONE = dict(rv=((NO_CANDIDATE, -1, 0, 0),) * 2, valid=((1, 0, 0),) * 4, mstate=((0, 0, 0, 1),) * 4)     # auto_rekey = 0: frame 0 is the only entry
_FULL = dict(rv=((NO_CANDIDATE, -1, 0, 0),) * 2, valid=((1, 1, 1),) * 4, mstate=((2, 4, 0, 5), (2, 4, 0, 5), (1, 5, 1, 6), (1, 5, 1, 6)))
# (step, auto_rekey) -> track: the flags of frames 0 .. 4; track5: those of frame 5, by seed where the seeds differ (as in TRACK_FLAGS_STUCK);
# rv: (flags, slot, links, grid) of the two revisits; valid / mstate: the entries' valid and (cur_slot, cur_links, cursor, serial) after the track of
# frame 4, the revisit on it, the track of frame 5 and the revisit on it
MAP_EXPECT = {
    # the restart empties the map and the bridge's re-key is stored alone with links 1: nothing to revisit at frame 4, itself one frame later
    ("1e13", 1): dict(track=(FIRST, EVERY, EVERY, EVERY, STOPPED | BRIDGED | REKEYED | RESTARTED), track5=EVERY, rv=((NO_CANDIDATE, -1, 0, 0), (ATTACHED, 0, 1, 64)),
                      valid=((1, 0, 0), (1, 0, 0), (1, 0, 1), (1, 0, 1)), mstate=((0, 1, 1, 5), (0, 1, 1, 5), (2, 2, 0, 6), (0, 1, 0, 6))),
    # the restart without a copy: the map is empty and the held keyframe outside it
    ("1e13", 0): dict(track=(FIRST, 0, 0, 0, STOPPED | BRIDGED | RESTARTED), track5={2: NO_START | RESTARTED, 5: STOPPED | RESTARTED}, rv=((NO_CANDIDATE, -1, 0, 0),) * 2,
                      valid=((0, 0, 0),) * 4, mstate=((-1, 0, 0, 1),) * 4),
    # a bridge far outside the image is chained in without a restart: the map stays valid and no entry is in view of the chain's h_origin_curr again
    ("1e12", 1): dict(track=(FIRST, EVERY, EVERY, EVERY, STOPPED | BRIDGED | REKEYED), track5=EVERY, **_FULL),
    ("1e12", 0): dict(track=(FIRST, 0, 0, 0, STOPPED | BRIDGED), track5={2: NO_START, 5: STOPPED}, **_ALONE),
    # 1e6 px is inside the domain of the map's inverse (3.2e6 px): the bridge's keyframe, stored 1e6 px out with links 4, is found again one frame later
    # (all 64 grid points) and the revisit attaches it.  Until the inverse judged its determinant in frame units this entry was refused like 1e12's.
    ("1e6", 1): dict(track=(FIRST, EVERY, EVERY, EVERY, STOPPED | BRIDGED | REKEYED), track5=EVERY, rv=((NO_CANDIDATE, -1, 0, 0), (ATTACHED, 2, 4, 64)),
                     valid=((1, 1, 1),) * 4, mstate=((2, 4, 0, 5), (2, 4, 0, 5), (1, 5, 1, 6), (2, 4, 1, 6))),
    ("1e6", 0): dict(track=(FIRST, 0, 0, 0, STOPPED | BRIDGED), track5={2: NO_START, 5: STOPPED | BRIDGED}, **_ALONE),
    # a step that cannot be composed is bridged by the previous key_px: the chain goes on and both revisits attach slot 0
    ("nan", 1): dict(track=(FIRST, EVERY, EVERY, EVERY, NO_START | BRIDGED | REKEYED), track5=EVERY, rv=((ATTACHED, 0, 0, 64),) * 2, valid=((1, 1, 1),) * 4,
                     mstate=((2, 4, 0, 5), (0, 0, 0, 5), (1, 1, 1, 6), (0, 0, 1, 6))),
    ("nan", 0): dict(track=(FIRST, 0, 0, 0, NO_START), track5=0, **_ALONE),
}


def map_flags(seed, name, auto_rekey):
    """the flags of the six track records of (b)"""
    e = MAP_EXPECT[name, auto_rekey]
    return e["track"] + (e["track5"][seed] if isinstance(e["track5"], dict) else e["track5"],)


def map_track_opts(auto_rekey):
    return K.opts(auto_rekey=auto_rekey, max_age=1 if auto_rekey else 0)


def run_map(seed, name, auto_rekey, track, revisit, after=None):
    """(b) on any session: track(frame, step, opts), revisit(frame, opts); after(i) is called after every call, i = 0 .. 7 -> (the six track records in
    frame order, the two revisit records)"""
    frames, steps = K.sequence("out-and-back", seed)[0], hostile_steps(seed, name, MAP_AT)
    to, ro = map_track_opts(auto_rekey), M.opts()
    after = after or (lambda i: None)
    recs, rvs = [], []
    for i in range(MAP_AT + 1):
        recs.append(track(frames[i], steps[i], to))
        after(i)
    rvs.append(revisit(frames[MAP_AT], ro))
    after(MAP_AT + 1)
    recs.append(track(frames[MAP_AT + 1], steps[MAP_AT + 1], to))
    after(MAP_AT + 2)
    rvs.append(revisit(frames[MAP_AT + 1], ro))
    after(MAP_AT + 3)
    return recs, rvs


def map_snapshots(i):
    """the index into MAP_EXPECT's valid / mstate of call i of run_map, or None for the tracks of frames 0 .. 3"""
    return i - MAP_AT if i >= MAP_AT else None


# ---- (c) relocalise: capacity 3, auto_rekey = 0, the 1e12 step at frame 2, so that key_px is 1e12 from there on; frame 3 with its true step; one
# relocalise on frame 3 (plain, or oriented under the 13 entries -36 .. 36 degrees of the 6-degree yaw table); frame 4 with its true step
RELOC_POISON, RELOC_AT = "1e12", 3
RELOC_KINDS = ("plain", "oriented")
RELOC_CASES = [(seed, kind) for seed in SEEDS for kind in RELOC_KINDS]
YAW13 = slice(24, 37)                      # of photo_search_oriented_util.yaw_table(lib): the 13 entries the existing oriented tests cut out
# seed -> the flags of the tracks of frames 0 .. 3 (the poisoned session, as TRACK_FLAGS_STUCK has it)
RELOC_TRACKS = {seed: TRACK_FLAGS_STUCK[RELOC_POISON, seed][:RELOC_AT + 1] for seed in SEEDS}
# The answer, for both seeds and both kinds: the search finds the held keyframe (frame 0; the map's only entry is its own slot), the alignment from
# the searched start passes, and RETRACKED overwrites the poisoned key_px with the record's offsets: (rv.flags, target, n_searched, n_found).  The
# track of frame 4 is then an ordinary tracked frame.
RELOC_ANSWER = (RETRACKED, _capi.RL_TARGET_HELD, 1, 1)
RELOC_NEXT = 0


def run_reloc(seed, track, relocalise):
    """(c) on any session: track(frame, step, opts), relocalise(frame, opts) -> (the track records of frames 0 .. 3, the relocalise's, frame 4's)"""
    frames, steps = K.sequence("out-and-back", seed)[0], hostile_steps(seed, RELOC_POISON, TRACK_AT)
    to, ro = track_opts(0), S.reloc_opts()
    recs = [track(frames[i], steps[i], to) for i in range(RELOC_AT + 1)]
    rl = relocalise(frames[RELOC_AT], ro)
    return recs, rl, track(frames[RELOC_AT + 1], steps[RELOC_AT + 1], to)
