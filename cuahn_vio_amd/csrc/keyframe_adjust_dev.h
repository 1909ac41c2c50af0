// keyframe_adjust_dev.h — the joint adjustment of a keyframe map (include/hnet.h hnet_op_keyframe_adjust_solve, hnet_op_keyframe_adjust,
// hnet_sessions_keyframe_adjust): what capi_keyframe_adjust.hip, keyframes_internal.h and kernels_keyframe_adjust.hip share.  The device compiles
// include/hnet_keyframe_adjust.h itself (host + device functions): pair_job, judge_edge, build, solve and finish are the functions
// tests/test_keyframe_adjust_cpu.py pins on the host.
#pragma once
#include "keyframe_map_dev.h"

#pragma clang force_cuda_host_device begin
#include "../../include/hnet_keyframe_adjust.h"
#pragma clang force_cuda_host_device end

namespace hnet {

using AdjustOpts = hnet_adjust::Opts;       // = hnet_keyframe_adjust_opts
using AdjustRec = hnet_adjust::Record;      // = hnet_keyframe_adjust
using AdjustEdge = hnet_adjust::Edge;       // = hnet_keyframe_adjust_edge
using AdjustJob = hnet_adjust::Job;
using AdjustJobs = hnet_adjust::JobTable;   // one session's jobs: {count, n_pairs, (i, j, grid, start_px) x 28}
constexpr int ADJUST_MAX_PAIRS = hnet_adjust::MAX_PAIRS, ADJUST_THREADS = 256, ADJUST_INFO = 64;
static_assert(sizeof(AdjustOpts) == sizeof(RobustOpts) + 80 && sizeof(AdjustJob) == 48 && sizeof(AdjustJobs) == 8 + 28 * 48 && sizeof(AdjustEdge) == 112 &&
              sizeof(AdjustRec) == 40 + 24 + 512 + 576 + 28 * 112 && sizeof(AdjustRec) % sizeof(double) == 0, "packed layouts");
static_assert(sizeof(hnet_adjust::Problem) <= 160 * 1024, "one session's Problem lives in the LDS of one workgroup");

// What is adjusted: the entries [n_sessions][capacity] and images [n_sessions][capacity][NPIX] of a map (capacity 1 .. 8; the operator-level calls are
// one session of m entries) and, for the sessions call, the sessions' states and map states (null: there are none to follow the entries)
struct AdjustSource { const uint8_t* img; MapEntry* entry; KeyState* state; const MapState* mstate; int n_sessions, capacity; };

// One wavefront per slot b < n (ids [n]: the sessions): lane p < 28 runs pair_job of pair p, the jobs are compacted in pair order with a ballot ->
// tab[b] (every byte written); rec[b] is zeroed but for n_jobs.  An id outside the table: no job.
hipError_t launch_keyframe_adjust_pairs(const int32_t* ids, int n, const AdjustSource& src, int min_grid, AdjustJobs* tab, AdjustRec* rec, hipStream_t s);
// One ROUND of the call's jobs, numbered through the slots in order: jobs first .. first + n_round - 1.  Grid (vectors, n_round), a uint4 per lane:
// prev[q] <- image [id][i], curr[q] <- image [id][j], x0[q] <- start_px (quiet NaNs, and nothing copied, for a job whose id or slots are out of range)
hipError_t launch_keyframe_adjust_gather(const int32_t* ids, int n, const AdjustSource& src, const AdjustJobs* tab, int first, int n_round, uint8_t* prev,
                                         uint8_t* curr, float* x0, hipStream_t s);
// One wavefront per job of the round, after the alignment (align_rec: the level-0 records [n_round]): judge_edge -> the job's row of rec[b].edge, the
// record's information matrix -> infos [n][28][64], and with edge_recs ([n][28], zeroed by the caller) the whole record
hipError_t launch_keyframe_adjust_edge(int n, const AdjustJobs* tab, int first, int n_round, const RobustRec* align_rec, const AdjustOpts& opts, AdjustRec* rec,
                                       double* infos, RobustRec* edge_recs, hipStream_t s);
// ONE workgroup of 256 lanes per slot: build, the whole Levenberg-Marquardt loop and finish of include/hnet_keyframe_adjust.h on the rows rec[b] holds
// (rec[b].n_jobs of them), infos [n][28][64] or null (identity); with opts.apply the entries, and the state of a session whose cur_slot moved, are
// rewritten.  rec[b]: every byte written.
hipError_t launch_keyframe_adjust_solve(const int32_t* ids, int n, const AdjustSource& src, const double* infos, const AdjustOpts& opts, AdjustRec* rec,
                                        hipStream_t s);

}  // namespace hnet
