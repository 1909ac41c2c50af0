/* hnet.h — C ABI of the MI355X-native HomographyNet inference path (libhnet_hip.so).
 *
 * Drop-in boundary for the reference class `pytorch::HomographyNet`
 * (reference cuahn_ros/homography_network/src/HomographyNet.h:23-67).  The header-only adapter
 * include/HomographyNet.h re-creates that class surface on top of these entry points; INTEGRATION.md shows
 * the binding.  No C++ / torch types cross this boundary: plain pointers, sizes and status codes; every
 * buffer is caller-owned.  One context per device; a context is NOT thread-safe (the reference object is
 * driven by a single ROS spin thread, ros_subscribe_cuahn.cpp:123-135).
 *
 * Conventions (reference model_to_trace.py:79-83, HomographyNet.cpp:160-165):
 *   images  : 224 rows x 320 cols, 8-bit gray (or float32 already scaled to [0,1])
 *   corners : ul, bl, br, ur ; each (u = column, v = row) ; 8 floats in that order
 *   mean    : total 4-corner offsets img1 -> img2 in pixels (includes the prior), float[8]
 *   cov     : 8x8 row-major, block diagonal of four 2x2 blocks, symmetric, float[64]
 *   err map : |warp(img2, H_total) - img1| * 255, clamped to [0,255] when emitted as u8
 */
#ifndef HNET_H
#define HNET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HNET_IMG_ROWS 224
#define HNET_IMG_COLS 320

/* status codes */
enum {
    HNET_OK = 0,
    HNET_ERR_INVALID_ARG = 1,
    HNET_ERR_BAD_WEIGHTS = 2,     /* missing / malformed HNETW001 blob */
    HNET_ERR_DEVICE = 3,          /* HIP runtime error (hnet_last_error has the text) */
    HNET_ERR_NOT_READY = 4,       /* fewer than two images pushed (HomographyNet.cpp:155-158) */
    HNET_ERR_CAPACITY = 5,        /* batch larger than max_batch; hnet_create: max_batch beyond what the kernels address (1 779 frame pairs per context) */
    HNET_ERR_UNSUPPORTED = 6
};

/* arithmetic of the conv contractions:
 *   HNET_PREC_FP32   exact fp32 MFMA (v_mfma_f32_32x32x2_f32), the reference's arithmetic
 *   HNET_PREC_BF16X3 fp32-grade accuracy on the bf16 matrix cores: every value is carried as three bf16 planes
 *                    (an exact split of its 24-bit significand) and each product is six bf16 MFMAs (csrc/igemm_s3.h)
 *   HNET_PREC_BF16   plain bf16 operands, fp32 accumulation: the same kernels reading ONE bf16 plane, one MFMA per product.
 *                    A REPORTED mode (BASELINE config 2 names "bf16"): ~2x the throughput at ~4e-3 .. 1e-1 px from the reference,
 *                    i.e. outside the 1e-4 px parity gate; tests/test_gpu_bf16_mode.py pins what it computes
 *   HNET_PREC_F16X2  fp32-grade accuracy on the fp16 matrix cores with THREE MFMAs per product: an activation is two fp16 planes
 *                    (a = A0 + A1 / 4096, 22 + 2 significand bits), a weight three (4096 w = W0 + W1, W0 / 4096), the accumulator
 *                    carries 4096 x the sum (csrc/s3_format.h).  Same parity gates as HNET_PREC_BF16X3.  Range: |weight| < 16
 *                    and |activation| < 32768 (guaranteed; up to 65520 all but 0.04 % of the values still split finitely, s3_format.h).
 *                    Outside it an overflow shows as a NON-FINITE result, never as a silently wrong one: the host-buffer entry points
 *                    (hnet_infer, hnet_infer_batch) then repeat the call in HNET_PREC_BF16X3 (hnet_precision below); the device-resident
 *                    entry points raise hnet_overflow_flag, which the caller polls after its own synchronisation */
enum { HNET_PREC_FP32 = 0, HNET_PREC_BF16 = 1, HNET_PREC_BF16X3 = 2, HNET_PREC_F16X2 = 3 };
enum { HNET_PIX_U8 = 0, HNET_PIX_F32 = 1 };        /* pixel format of image buffers */

/* Replaces: the variant choice the reference bakes into the traced .pt file
 * (trace_pytorch_model/trace_model.py:36-46; blocks_to_run model_to_trace.py:72; MC_dropout_num :202;
 * dropout_rate trace_model.py:16; "_showError" HomographyNet.cpp:96-100). */
/* use_prior, blocks_to_run, mc_samples, emit_error_map = HNET_FROM_FILE (dropout_p: any negative value): hnet_create takes the field from the blob's
 * `hnet.variant` record (python -m cuahn_vio_amd.weights --variant ...: one blob per traced variant, as the reference has one .pt per variant); a blob
 * without the record gives the reference's launch values (use_prior 1, blocks_to_run 3, N 16, p 0.05, no error map).  hnet_get_config returns what is in effect. */
#define HNET_FROM_FILE (-1)
typedef struct hnet_config {
    uint32_t struct_size;      /* sizeof(hnet_config), for forward compatibility */
    int32_t  device_id;        /* HIP device ordinal */
    int32_t  use_prior;        /* 0: full 4-block model.  1: H0 = DLT(prior), then `blocks_to_run` part-1 blocks, then block 4 */
    int32_t  blocks_to_run;    /* 1..3, the reference attribute (3 = "traced_model_3_blocks_using_prior"); used only with prior */
    int32_t  mc_samples;       /* N of the MC-dropout ensemble (reference 16) */
    float    dropout_p;        /* drop probability (reference 0.05); 0 = deterministic */
    uint64_t mc_seed;          /* key of the mask function, include/hnet_rng.h */
    int32_t  emit_error_map;   /* 1: "_showError" variant, the photometric error map is computed */
    int32_t  precision;        /* HNET_PREC_*; hnet_default_config: HNET_PREC_F16X2 */
    int32_t  max_batch;        /* capacity (frame pairs) of the persistent activation buffers, >= 1 */
    int32_t  mc_sample_begin;  /* this context evaluates global samples [begin, end) in the *_partial entry points; */
    int32_t  mc_sample_end;    /* 0,0 = all */
    /* Kernel selection (round 4: the library reads no environment variable; 0 everywhere = the measured defaults = what hnet_default_config sets).
     * These fields replace the HNET_* switches that rounds 1 - 3 read with getenv at hnet_create: a stray variable in a deployment can no longer
     * change kernels or summation order.  The tests and tools/ab_bench.py set them explicitly (the Python mirror maps its own environment onto them). */
    int32_t  warp_exact;       /* 1: the warp keeps grid_sample's sampling positions bit for bit (warp.py:70); 0: fast sampler, positions within 1.3e-4 px (measured) */
    int32_t  graph;            /* HNET_GRAPH_*: hipGraph replay of the batch-1 forward of hnet_infer */
    uint32_t variant;          /* HNET_VARIANT_*: reference kernels for in-process A/B measurements and the bitwise cross-kernel tests */
} hnet_config;

enum { HNET_GRAPH_DEFAULT = 0 /* replay */, HNET_GRAPH_OFF = 1 /* eager launches */, HNET_GRAPH_TIMING = 2 /* replay, also inside hnet_time_batch_device */ };
enum {
    HNET_VARIANT_GEMM_MASK = 0xff,            /* low byte: implicit-GEMM kernel selection (csrc/s3_dispatch.h); an unknown code is HNET_ERR_INVALID_ARG:
                                                  0 = defaults; 13 = heads FC1 on the four-wave 128 x 64 kernel; 22 = on the eight-wave kernel of round 3;
                                                  20 = conv layers on the four-wave lean kernels (no pipelined LDS-DMA / region kernels); 21 = the pipelined and the
                                                  region kernel at any batch (tests); 25 = no region kernel; 30 = split-K layers with splitk_reduce launches and the
                                                  split-K heads at every batch (the round-4 latency path: A/B and bitwise tests of round 5) */
    HNET_VARIANT_NO_LATENCY_PATH = 1u << 8,   /* batch <= 8 on the multi-launch path (bit-identical; tests/test_gpu_latency_path.py) */
    HNET_VARIANT_UNFUSED_B3 = 1u << 9,        /* block_3_0 and block_3_1 as separate launches (fp16-plane mode) */
    HNET_VARIANT_UNFUSED_B42 = 1u << 10,      /* block_4_2 and block_4_3 as separate launches (fp16-plane mode) */
    HNET_VARIANT_NO_CHAIN = 1u << 11,         /* batch <= 8: the tail layers of every block as separate launches instead of the one-XCD chain launch of round 6
                                                  (csrc/chain_lat.h; fp16-plane mode; same arithmetic, another summation order: results agree to fp32 rounding) */
    HNET_VARIANT_CHAIN_GRID_8 = 1u << 12,     /* tests: the chain launches with 8 workgroups instead of 256 (fewer resident workgroups than items: every workgroup works
                                                  through several items of a layer) and */
    HNET_VARIANT_CHAIN_GRID_3 = 1u << 13,     /* with 3 (XCDs without a workgroup: pairs are picked up by whoever is done) - the same bits as the 256-workgroup launch */
    HNET_VARIANT_GRAPH_COPIES = 1u << 15,     /* hnet_infer's graph moves {sequence number, prior} and {mean, cov, error map, flag} with memcpy nodes, as until round 6, instead of
                                                  letting the kernels read / write the pinned host block directly (A/B and tests; same results) */
    HNET_VARIANT_CHAIN_NO_FC = 1u << 16,      /* batch <= 8: the block-tail Linear(5120, 8) recomputed by every workgroup of the next warp + pool launch (rounds 3 - 5) instead of
                                                  summed from the 32 partial sums the tail chain's last layer leaves (round 6; another summation order: fp32 rounding) */
    HNET_VARIANT_WARP_FUSE = 1u << 14         /* batch > 8: block 4's warp + concat sampled INSIDE the block_4_0 + block_4_1 kernel (csrc/conv_b4_fused.h WARPIN, round 6; fp16-plane
                                                  mode, 4-byte aligned u8 images) instead of a launch of its own that writes the padded fp16 planes.  Same sampler, same bits
                                                  (tests/test_gpu_warp_fuse.py) - and 0.10 ms per 256 pairs SLOWER (the sampling sits in every workgroup's own timeline:
                                                  profiles/r06_experiments_not_shipped.log item 15), so it is opt-in, not the default */
};

typedef struct hnet_ctx hnet_ctx;

typedef struct hnet_timing {
    double device_ms;          /* "pure network inference": device time of the last forward (HomographyNet.cpp:178-188) */
    double host_ms;            /* wall time of the last hnet_infer / hnet_infer_batch call, incl. H2D and D2H */
    int64_t n_inferences;      /* every forward of hnet_infer / hnet_infer_batch (also the mask sequence number of hnet_infer) */
    double sum_device_ms_after_100;   /* running sum over the iteration == 0 calls that skips the first 100 (HomographyNet.cpp:245-251) */
    int64_t n_main_inferences; /* `inference_counting` (HomographyNet.cpp:189): calls with iteration == 0 only */
} hnet_timing;

/* fills `cfg` with the reference's launch defaults — full model, N=16, p=0.05, max_batch 1 — and precision =
 * HNET_PREC_F16X2 (fp32-grade results on the fp16 matrix cores; passes the same parity gates as HNET_PREC_BF16X3 and as
 * HNET_PREC_FP32, which is the reference's own fp32 arithmetic; both stay selectable) */
void hnet_default_config(hnet_config* cfg);

/* Replaces HomographyNet::load_network_model (HomographyNet.cpp:81-103): `weights_path` names an HNETW001
 * blob (cuahn_vio_amd/weights.py) instead of a TorchScript .pt.  Also runs the warm-up forward the reference
 * constructor does (HomographyNet.cpp:28-45). */
int hnet_create(const hnet_config* cfg, const char* weights_path, hnet_ctx** out);
int hnet_create_from_memory(const hnet_config* cfg, const void* blob, size_t len, hnet_ctx** out);
void hnet_destroy(hnet_ctx* ctx);

const char* hnet_status_string(int status);
const char* hnet_last_error(const hnet_ctx* ctx);   /* text of the last HNET_ERR_DEVICE etc.; never NULL */
const char* hnet_version(void);
/* Device-resident entry points and the fp16-plane range.  Every forward ORs bit 0 of a device word when one of its outputs (mean / cov, or
 * the per-sample head outputs of the *_partial path) is not finite; this call synchronises `stream` (NULL = the context's), returns the word in
 * *flags and clears it.  In HNET_PREC_F16X2 a set bit with finite inputs means an activation left the fp16-plane range: run that batch
 * again on a HNET_PREC_BF16X3 context (same results as fp32 arithmetic, fp32 range).  Costs no extra launch. */
int hnet_overflow_flag(hnet_ctx* ctx, void* stream, int* flags);

/* the arithmetic mode in effect (HNET_PREC_*).  It differs from the requested one in two cases, both HNET_PREC_F16X2 -> HNET_PREC_BF16X3
 * (same results, twice the matrix-core work): a weight >= 16 at hnet_create, or an activation beyond the fp16 range seen by hnet_infer /
 * hnet_infer_batch (non-finite outputs): the context re-packs its weights, repeats the call and stays in HNET_PREC_BF16X3.  The
 * device-resident entry points cannot look at their results: there such an overflow shows as non-finite outputs and raises
 * hnet_overflow_flag.  A non-finite INPUT (NaN prior from a diverged filter, NaN float image) is not an overflow: the call returns
 * the non-finite outputs as the reference would and the context keeps its mode. */
int hnet_precision(const hnet_ctx* ctx);
/* the configuration in effect: HNET_FROM_FILE fields resolved from the blob, defaults filled in (what a deployment logs next to the file name) */
int hnet_get_config(const hnet_ctx* ctx, hnet_config* out);

/* Replaces HomographyNet::load_current_img (HomographyNet.cpp:127-151): copies the 224x320 8-bit image
 * (row_stride in bytes) to the device, prev <- curr, curr <- img; counts images; records `t` from the second
 * image on. */
int hnet_push_image(hnet_ctx* ctx, const uint8_t* data, int rows, int cols, int row_stride, double t);

/* The reference's IEKF keeps a SECOND traced model for iteration > 0 (`HomographyNet_model_iterative`, loaded from network_model_iterative_path when
 * num_of_iteration > 1: HomographyNet.cpp:20-24,104-124, run at :209-219) - a separate file that may be another variant (fewer blocks).  Both
 * modules see the same nn_inputs (:160-172).  hnet_attach_images makes `ctx` (the iterative model's context) read the frame pair, the image counter,
 * the time stamp and the MC-dropout sequence number of `source` (the main model's context, same device): images are pushed to `source` only, and
 * hnet_infer(ctx, ...) runs on source's current pair with the next sequence number of the shared count.  `source` must outlive `ctx`. */
int hnet_attach_images(hnet_ctx* ctx, hnet_ctx* source);
int hnet_image_count(const hnet_ctx* ctx);             /* the public `img_counter` (HomographyNet.h:33) */

/* ---- image pre-processing ahead of load_current_img --------------------------------------------
 * The reference undistorts and resizes the raw camera image on the CPU before handing it to the network:
 * CamBase::initialize_undist_map / initialize_undist_map_fisheye build two 224x320 float maps with
 * cv::initUndistortRectifyMap / cv::fisheye::initUndistortRectifyMap towards the virtual camera f = 159.5,
 * c = (159.5, 111.5) (ov_core/src/cam/CamBase.h:165-180) and undistort_and_resize_img is cv::remap(INTER_LINEAR)
 * (:182-186), called from VioManager.cpp:184.  Here the maps are built once on the host with the published
 * formulas of those two OpenCV functions and the remap is a HIP kernel that writes straight into the context's image
 * ring, so a raw frame goes host -> device once and never comes back.
 * PARITY UNPINNED: OpenCV is neither in this image nor vendored by the reference and the reference holds no vectors
 * for this step.  The kernel interpolates with sample positions quantised to 1/32 px like cv::remap (INTER_BITS = 5)
 * in exact integer arithmetic.  Deviation class against cv::remap, exactly: OpenCV blends with a 32 x 32 table of 15-bit coefficients
 * (INTER_REMAP_COEF_BITS = 15: each 1-D weight k/32 is rounded into a pair that sums to 32768) and rounds the 2-D sum once, this
 * kernel blends with the exact products (32 - fx)(32 - fy) ... fx fy / 1024 and rounds half up: same sample positions, same four
 * taps, a result that can differ by ONE grey level where the exact blend sits within 2^-10 of a rounding boundary; and OpenCV's maps
 * pass through its fixed-point convertMaps, whose rounding of positions exactly half way between two 1/32-px steps may pick the other
 * step (again <= one grey level at a unit gradient).  What IS pinned: bit-exactness against the numpy restatement under tests (see tests/test_undistort.py), four analytic
 * map properties, and an end-to-end property independent of the restated formulas - the remap of an independently simulated fisheye
 * photograph of an analytic scene recovers the scene to 0.34 grey levels RMS, 1.0 max (tests/test_undistort.py). */
typedef struct hnet_camera {
    int32_t fisheye;           /* 1: equidistant model (cam0_is_fisheye, uzhfpv.launch:77), 0: radial-tangential */
    int32_t raw_rows, raw_cols;/* size of the raw image (cam0_wh, uzhfpv.launch:75: 640 x 480) */
    double  k[4];              /* fx, fy, cx, cy (cam0_k) */
    double  d[4];              /* fisheye: k1..k4; radtan: k1, k2, p1, p2 (cam0_d) */
} hnet_camera;
/* builds and uploads the maps for `cam` (initialize_undist_map[_fisheye]) */
int hnet_set_camera(hnet_ctx* ctx, const hnet_camera* cam);
/* or supplies them directly (the reference's undist_map1 / undist_map2: 224x320 float each, x and y source coordinates) */
int hnet_set_undistort_maps(hnet_ctx* ctx, const float* map_x, const float* map_y, int raw_rows, int raw_cols);
/* copies the maps in use back (224x320 floats each) */
int hnet_get_undistort_maps(hnet_ctx* ctx, float* map_x, float* map_y);
/* undistort_and_resize_img + load_current_img: raw 8-bit image (row_stride in bytes) -> remap on the device -> image ring */
int hnet_push_raw_image(hnet_ctx* ctx, const uint8_t* raw, int rows, int cols, int row_stride, double t);
/* operator-level: the remapped 224x320 image back on the host (parity tests) */
int hnet_op_undistort(hnet_ctx* ctx, const uint8_t* raw, int rows, int cols, int row_stride, uint8_t* out);
double hnet_latest_time(const hnet_ctx* ctx);          /* get_latest_inference_time() (HomographyNet.h:31) */

/* Replaces HomographyNet::network_inference (HomographyNet.cpp:153-252) on (prev, curr).
 * prior_px: 8 doubles (pixels) — required when the context was created with use_prior, else ignored/NULL.
 * iteration: IEKF iteration index; >0 selects the reference's "iterative" model, which is the same network
 *            run again with the updated prior, so it is accepted and otherwise ignored.
 * err_map_out: NULL or 224*320 bytes (needs emit_error_map).  Returns HNET_ERR_NOT_READY before 2 images. */
int hnet_infer(hnet_ctx* ctx, const double* prior_px, int iteration,
               float mean_out[8], float cov_out[64], uint8_t* err_map_out);

/* Batched frame pairs, host buffers: prev/curr [B][224][320] (pix_fmt), prior [B][8] floats or NULL,
 * pair_seq0 = sequence number of pair 0 (pair b uses pair_seq0 + b in the mask key),
 * mean [B][8], cov [B][64], err_map [B][224][320] float or NULL.  Semantics = the batch-1 reference applied
 * independently to each pair (the reference itself is batch-1 only, warp.py:64). */
int hnet_infer_batch(hnet_ctx* ctx, const void* prev, const void* curr, int pix_fmt, const float* prior,
                     int batch, uint64_t pair_seq0, float* mean, float* cov, float* err_map);

/* Same with every buffer resident in device memory; enqueues on `stream` (a hipStream_t) and does not synchronise.
 * NULL = the context's own (non-blocking) stream; to enqueue on HIP's legacy default stream pass hipStreamLegacy
 * ((hipStream_t)1) — the handle 0 some frameworks report for it cannot be told apart from NULL. */
int hnet_infer_batch_device(hnet_ctx* ctx, const void* d_prev, const void* d_curr, int pix_fmt,
                            const float* d_prior, int batch, uint64_t pair_seq0,
                            float* d_mean, float* d_cov, float* d_err_map, void* stream);

/* The same forward with PACKED outputs: d_out72 [batch][72] fp32, record of pair b = mean (8 corner offsets) followed by the row-major 8 x 8 covariance
 * (64).  This is the message a multi-GPU caller exchanges (one ncclAllGather / all_gather_into_tensor of batch x 288 bytes per rank:
 * tests/cpp/rccl_gather_example.cpp, cuahn_vio_amd/dist.py); written directly by the ensemble kernel, no packing copies.  Bit-identical values. */
#define HNET_PACKED_FLOATS 72
int hnet_infer_batch_packed_device(hnet_ctx* ctx, const void* d_prev, const void* d_curr, int pix_fmt, const float* d_prior, int batch,
                                   uint64_t pair_seq0, float* d_out72, float* d_err_map, void* stream);

/* MC-dropout sharding: the trunk runs on every rank, the heads only for this context's
 * global samples [mc_sample_begin, mc_sample_end).  Outputs per pair: mean_s / logvar_s
 * [B][n_local][8] and H_part1 [B][9].  After gathering all N samples (rank order = sample order) the
 * ensemble is finished with hnet_mc_finish_device in the reference's two-pass order
 * (model_to_trace.py:274-280). */
int hnet_infer_mc_partial_device(hnet_ctx* ctx, const void* d_prev, const void* d_curr, int pix_fmt,
                                 const float* d_prior, int batch, uint64_t pair_seq0,
                                 float* d_mean_s, float* d_logvar_s, float* d_h_part1, void* stream);
int hnet_mc_finish_device(hnet_ctx* ctx, const float* d_mean_s, const float* d_logvar_s, int n_total,
                          const float* d_h_part1, int batch, float* d_mean, float* d_cov, void* stream);
/* ... with the packed [batch][72] record of hnet_infer_batch_packed_device as output */
int hnet_mc_finish_packed_device(hnet_ctx* ctx, const float* d_mean_s, const float* d_logvar_s, int n_total, const float* d_h_part1,
                                 int batch, float* d_out72, void* stream);
/* Round 5 (BASELINE config 4 without layout launches): the ensemble straight from the buffer an all-gather fills.  Every rank passes ONE [2][B][n_local][8]
 * array to hnet_infer_mc_partial_device (d_mean_s = its first half, d_logvar_s = its second) and all-gathers it into d_gathered [world][2][B][n_local][8]
 * (ncclAllGather / all_gather_into_tensor: rank-major = global sample order); this call reads sample s of pair b at rank s / n_local - no stack, permute or
 * copy between the collective and the finish.  Same two-pass arithmetic and the same bits as hnet_mc_finish_packed_device on the re-ordered samples. */
int hnet_mc_finish_gathered_device(hnet_ctx* ctx, const float* d_gathered, int world, int n_local, const float* d_h_part1, int batch, float* d_out72,
                                   void* stream);

/* ---- context groups (round 6): INDEPENDENT steps on several contexts ------------------------------------------------------------
 * A forward of <= 64 frame pairs leaves most of the chip waiting on its own chain of dependent launches.  Where the steps are independent - a server's batches,
 * a rank's share of a streamed sequence (BASELINE configs 3 and 5) - issuing them round-robin on a few contexts, each with its own HIP stream and buffers, runs
 * one step's chain under the others' kernels: + 30 ... 40 % pairs/s at 32 - 64 pairs per step, + 5 % at 256 (bench.py --contexts).
 * A group is n_ctx contexts of ONE configuration on one device (weights uploaded per member).  It creates its streams before anything else, in a fixed order,
 * each on its own stream-priority level as far as the device has levels (three on this part): streams of one priority share the runtime's hardware queues in an
 * order that depends on the process's stream history, and two members on one queue serialise; queues of different priority are never shared.
 * hnet_group_infer_batch_packed_device = hnet_infer_batch_packed_device on member (call count mod n_ctx), on THAT member's stream; it does not synchronise.
 * Outputs of consecutive calls must not alias (two steps are in flight at once).  hnet_group_join makes `stream` wait for everything enqueued on the members so far
 * (one event per member); hnet_group_synchronize waits on the host.  Results are those of a single context, bit for bit (tests/test_gpu_group.py).
 * Not thread-safe (one caller thread, like a context). */
#define HNET_GROUP_MAX 8
typedef struct hnet_group hnet_group;
int hnet_create_group(const hnet_config* cfg, const char* weights_path, int n_ctx, hnet_group** out);
int hnet_create_group_from_memory(const hnet_config* cfg, const void* blob, size_t len, int n_ctx, hnet_group** out);
void hnet_destroy_group(hnet_group* group);
int hnet_group_size(const hnet_group* group);
hnet_ctx* hnet_group_context(hnet_group* group, int i);      /* member i (hnet_get_config, hnet_precision, per-member calls); owned by the group */
void* hnet_group_stream(hnet_group* group, int i);           /* member i's hipStream_t (to order a caller's own work - a collective, a copy - behind its step) */
const char* hnet_group_last_error(const hnet_group* group);
/* member: NULL, or receives the index of the member the step was enqueued on */
int hnet_group_infer_batch_packed_device(hnet_group* group, const void* d_prev, const void* d_curr, int pix_fmt, const float* d_prior, int batch,
                                         uint64_t pair_seq0, float* d_out72, float* d_err_map, int* member);
int hnet_group_join(hnet_group* group, void* stream);
int hnet_group_synchronize(hnet_group* group);
int hnet_group_overflow_flag(hnet_group* group, int* flags);   /* hnet_overflow_flag of every member, ORed; synchronises the members */

/* ---- sessions: many camera streams on ONE context ----------------------------------------------------------------------------------
 * The reference runs one HomographyNet object per camera: one frame ring (load_current_img, HomographyNet.cpp:127-151), one mask sequence count (the
 * forward's call count, :153-252) and one undistort camera (CamBase.h:165-186) each.  A sessions object keeps that state for n_sessions cameras on one context
 * and runs the pairs of any subset of them as ONE batched forward: session i's result is what a dedicated context with the same blob and config gives when
 * driven by hnet_push_image / hnet_push_raw_image + hnet_infer (pair b's mask key = its session's own count: hnet_infer_batch_seqs_packed_device).
 * Device ring: n_sessions x 2 frames.  `ctx` must outlive the sessions; errors go to hnet_last_error(ctx); a failed call changes no state.
 * Session calls never touch the context's own image ring, counters or timing (hnet_infer on the same context keeps its sequence).
 * ids: n distinct session indices.  HNET_ERR_INVALID_ARG: an id out of range or repeated, an unbound camera, a raw size other than the bound camera's, an error
 * map without emit_error_map; HNET_ERR_NOT_READY: a listed session holds fewer than two images; HNET_ERR_CAPACITY: n > max_batch; HNET_ERR_UNSUPPORTED
 * (hnet_create_sessions): a context that evaluates a sample shard (mc_sample_begin / end != 0, 0).  Not thread-safe (one caller thread, like a context). */
typedef struct hnet_sessions hnet_sessions;
int  hnet_create_sessions(hnet_ctx* ctx, int n_sessions, hnet_sessions** out);
void hnet_destroy_sessions(hnet_sessions* s);
/* load_current_img (HomographyNet.cpp:127-151) for n sessions at once: frame i = 224 x 320 u8 at frames + i frame_stride (row_stride bytes per row) goes to
 * session ids[i]; prev <- curr, counts, t[i] recorded from the second image on (t NULL: times not recorded).  The frames are copied into pinned staging
 * (double-buffered, not retained), uploaded with one copy and scattered into the ring by one launch; no synchronisation. */
int  hnet_sessions_push(hnet_sessions* s, int n, const int32_t* ids, const uint8_t* frames, int row_stride, size_t frame_stride, const double* t);
/* initialize_undist_map[_fisheye] (CamBase.h:165-180) for one more camera; maps built exactly as hnet_set_camera builds them.  *cam_id receives its index */
int  hnet_sessions_add_camera(hnet_sessions* s, const hnet_camera* cam, int* cam_id);
int  hnet_sessions_bind_camera(hnet_sessions* s, int id, int cam_id);
/* undistort_and_resize_img (CamBase.h:182-186) + load_current_img for n sessions: raw frame i (rows x cols u8, row_stride bytes per row) at raw + i frame_stride
 * remapped with session ids[i]'s camera straight into its ring slot (the bits of hnet_push_raw_image); one upload, one launch, no synchronisation */
int  hnet_sessions_push_raw(hnet_sessions* s, int n, const int32_t* ids, const uint8_t* raw, int rows, int cols, int row_stride, size_t frame_stride,
                            const double* t);
/* network_inference (HomographyNet.cpp:153-252) on the current pair of each listed session, as one batched forward: prior_px [n][8] doubles (pixels; required
 * with use_prior), mean [n][8], cov [n][64], err_map [n][224][320] u8 or NULL.  Each listed session's sequence number advances by one (an IEKF re-run is
 * another call with the new priors).  One synchronisation; the F16X2 overflow repeat of hnet_infer_batch applies (same keys, counts advance once). */
int  hnet_sessions_infer(hnet_sessions* s, int n, const int32_t* ids, const double* prior_px, float* mean, float* cov, uint8_t* err_map);
/* The IEKF's second model (network_model_iterative_path, HomographyNet.cpp:20-24,104-124,209-219; hnet_attach_images for one camera) for every session:
 * `iter` is a context created from the iterative weight file (it may be another variant, e.g. prior-1, N = 8, p = 0.1); it needs no frames of its own - its
 * forwards read the pairs the sessions' ring holds - and while attached it is dedicated to these sessions: its forwards are enqueued on the sessions'
 * context's stream.  iter = NULL detaches.  `iter` must outlive the attachment.  HNET_ERR_INVALID_ARG (nothing changes): iter is the sessions' own context,
 * lives on another device, has another use_prior than the main model, or a smaller max_batch; HNET_ERR_UNSUPPORTED: iter evaluates a sample shard. */
int  hnet_sessions_set_iterative_model(hnet_sessions* s, hnet_ctx* iter);
/* hnet_sessions_infer for IEKF iteration `iteration` (>= 0): iteration 0 is exactly hnet_sessions_infer; iteration > 0 runs the attached iterative model, or
 * the main model when none is attached (as hnet_infer accepts the index).  Each listed session's sequence number advances by one whichever model ran: the
 * adapter's one shared count.  err_map needs emit_error_map on the context that runs.  An F16X2 overflow demotes that context. */
int  hnet_sessions_infer_iter(hnet_sessions* s, int iteration, int n, const int32_t* ids, const double* prior_px, float* mean, float* cov, uint8_t* err_map);
int  hnet_sessions_image_count(const hnet_sessions* s, int id);           /* img_counter (HomographyNet.h:33) of session id; -1 for a bad id */
double hnet_sessions_latest_time(const hnet_sessions* s, int id);         /* get_latest_inference_time() (HomographyNet.h:31); -1 before the second image */
int  hnet_sessions_set_seq(hnet_sessions* s, int id, uint64_t seq);       /* next mask sequence number of session id (default 0) */
uint64_t hnet_sessions_seq(const hnet_sessions* s, int id);
int  hnet_sessions_reset(hnet_sessions* s, int id);                       /* camera restarted: image count 0, time -1, sequence number kept */
int  hnet_sessions_get_frame(hnet_sessions* s, int id, int which /* 0 prev, 1 curr */, uint8_t* out);   /* operator level (tests): 224 x 320 bytes */
int  hnet_sessions_last_timing(const hnet_sessions* s, hnet_timing* out); /* the sessions' own: last infer's device / host ms, infer calls so far */
/* hnet_infer_batch_packed_device with one mask sequence number per pair: d_pair_seq [batch] uint64 in device memory (pair b's key = d_pair_seq[b] instead of
 * pair_seq0 + b).  The table [s0, s0 + 1, ...] gives the bits of pair_seq0 = s0. */
int  hnet_infer_batch_seqs_packed_device(hnet_ctx* ctx, const void* d_prev, const void* d_curr, int pix_fmt, const float* d_prior, int batch,
                                         const uint64_t* d_pair_seq, float* d_out72, float* d_err_map, void* stream);

/* ---- filters: one 27-state filter per session, stepped on the device ------------------------------------------------------------------
 * The per-frame filter work of VioManager.cpp:188-275 for any subset of a sessions object's cameras, on the context's stream, with ONE host synchronisation:
 * IMU propagation of mean and covariance (Propagator.cpp:28-76), the prior (:230-234), max_iekf_iteration batched forwards each followed by
 * UpdaterHNet::update under the reference's gate (:257: latest time == t_frame and image count > 10), then State::reset_4pt_offset (:275).
 * For every listed session a step equals hnet_ekf::propagate_with_imu + hnet_ekf::iterated_update (include/hnet_ekf.h) around a dedicated context; each
 * forward advances the session's mask sequence number by one, as max_iekf_iteration calls of hnet_sessions_infer do.  Unlisted sessions are untouched.
 * The IMU readings are selected on the host (hnet_ekf::select_imu_readings), everything else runs on the device.  The one difference to the host loop:
 * a singular innovation covariance leaves that session's state as it was before that update and skips its later updates in the step (updates[i] < 0),
 * where hnet_ekf::iterated_update stops iterating; the device still runs the later batched forwards for it, so its sequence number advances once per
 * iteration either way.  Errors (the hnet_sessions codes: a bad or repeated id, n > max_batch, a session with fewer than two images, t_frame <= state t)
 * change no state.  The F16X2 overflow and chain-timeout repeats of hnet_sessions_infer apply to the whole step (the listed states are restored first).
 * Iteration routing: with an iterative model attached to the sessions (hnet_sessions_set_iterative_model) and max_iekf_iteration > 1, forward 0 of a step
 * runs on the main context and forwards 1 .. max_iekf_iteration - 1 on the iterative one, as hnet_sessions_infer_iter would route them; still one upload,
 * one download and one synchronisation, and the frame pairs are gathered once.  A repeat then acts on the context that asked for it: a chain time-out sends
 * the context that flagged it back to the launches, an overflow demotes the context whose forward overflowed (the first forward with non-finite outputs
 * of finite priors: forward 0 -> main, later -> iterative), and the whole step reruns from the untouched states; sequence numbers advance once per accepted
 * step.  With max_iekf_iteration = 1 or nothing attached a step is what it is without the attachment, bit for bit.
 * The filters must be destroyed before their sessions. */
typedef struct hnet_imu { double t, wm[3], am[3]; } hnet_imu;
/* defaults (hnet_filter_default_params): uzhfpv.launch - indoor T_ItoCmono (:84-89; i_t_i2c = -c_R_i^T t, State.cpp:95-96), noise densities
 * (:69-72), gravity (:48), up_linear_K_HNet_Cov 10 (:65), imu_avg (use_imuavg, :37).  cam_imu_dt: the fixed camera-IMU time offset (t_imu = t_cam + dt);
 * its default 0 is NOT the launch value (uzhfpv.launch:43 sets calib_camimu_dt = -0.0148489, applied as a fixed offset): set it for that setup */
typedef struct hnet_filter_params {
    double c_R_i[9], i_t_i2c[3];
    double sigma_w, sigma_a, sigma_wb, sigma_ab, gravity_mag, k_net_cov, cam_imu_dt;
    int32_t imu_avg;
} hnet_filter_params;
/* t: time of the state (camera clock); p, q (Hamilton w, x, y, z), v, ba, bg, offset (ul, bl, br, ur; x, y, z each), cov 27 x 27 row major
 * (the hnet_ekf::State layout behind t).  A new filter: t = 0, q = identity, everything else 0. */
typedef struct hnet_filter_state { double t, p[3], q[4], v[3], ba[3], bg[3], offset[12], cov[729]; } hnet_filter_state;
typedef struct hnet_filters hnet_filters;

void hnet_filter_default_params(hnet_filter_params* p);
/* one filter per session of `s`, all with the default parameters; max_iekf_iteration forwards per step, 1 .. 64 (HNET_ERR_INVALID_ARG otherwise;
 * uzhfpv.launch:67: 1) */
int  hnet_create_filters(hnet_sessions* s, int max_iekf_iteration, hnet_filters** out);
void hnet_destroy_filters(hnet_filters* f);
int  hnet_filters_set_params(hnet_filters* f, int id, const hnet_filter_params* p);
int  hnet_filters_set_state(hnet_filters* f, int id, const hnet_filter_state* st);
int  hnet_filters_get_state(hnet_filters* f, int n, const int32_t* ids, hnet_filter_state* out);
/* one frame for n sessions: t_frame [n] (camera clock, > each state's t); session ids[i]'s readings are imu[imu_off[i] .. imu_off[i + 1]) in time order (a window
 * around [state t, t_frame], as VioManager's imu_data).  state_out [n] (the states after the step), net_out [max_iekf_iteration][n][72] (packed mean | cov of
 * every forward) and updates [n] (updates applied; -1 - applied when a singular S stopped them) may be NULL. */
int  hnet_filters_step(hnet_filters* f, int n, const int32_t* ids, const double* t_frame, const hnet_imu* imu, const int64_t* imu_off,
                       hnet_filter_state* state_out, float* net_out, int32_t* updates);
/* the fp32 priors [max_iekf_iteration][n][8] the forwards of the last step read (whether or not use_prior let them); n must be that step's n
 * (HNET_ERR_INVALID_ARG otherwise, nothing written) (tests, tools) */
int  hnet_filters_last_priors(const hnet_filters* f, int n, float* out);
int  hnet_filters_last_timing(const hnet_filters* f, hnet_timing* out);   /* last step: device ms (upload end .. last update), host ms; steps so far */

/* ---- filters, fed: device IMU rings, the static initialiser, one call that advances every camera that is ready ----------------------------
 * The front half of VioManager for the filters above: readings are handed over once (feed_measurement_imu), kept in a device ring per session, and
 * hnet_filters_advance is track_image_and_update (VioManager.cpp:155-275) for the listed sessions with ONE host synchronisation: the window selection
 * (Propagator.cpp:81-175), the initialiser (InertialInitializer.cpp:163-279 + StateHelper.cpp:35-61; hnet_ekf::initialize_with_imu / initialize_cov) and
 * the propagation run on the device, the forwards of the sessions that step run as one batch.  hnet_filters_step stays usable next to these calls and
 * ignores the rings.
 * Per listed session, t_frame is the stamp of its latest hnet_sessions_push[_raw] (a push without stamps leaves it without a frame):
 *   HNET_ADV_NO_FRAME     no frame newer than the state's time (or than the last frame the initialiser dropped).  Nothing changes.
 *   HNET_ADV_WAIT_IMU     no reading newer than the frame yet: newest reading's t - cam_imu_dt <= t_frame (VioManager.cpp:148-149).  Nothing changes.
 *   HNET_ADV_WAIT_INIT    not initialised and the initialiser refuses the ring's readings.  The frame is dropped (the reference returns before
 *                         load_current_img, :158-162): the session's image count restarts at 0, the filter's state is untouched.
 *   HNET_ADV_INITIALIZED  the initialiser accepted: state = time0 / the initial mean / initialize_cov, this frame is image 1 of the session, and the
 *                         state is propagated from time0 to t_frame with the offsets reset (no forward).  time0 is an IMU-clock time that the
 *                         reference uses as the state's camera-clock time (:341); so do we.  If time0 > t_frame the frame is out of order
 *                         (:203-206): the state stays at time0 and later frames up to time0 report NO_FRAME.
 *   HNET_ADV_PROPAGATED   initialised, fewer than two images: propagated, offsets reset, no forward (HomographyNet.cpp:155-158; the mask sequence
 *                         number does not advance).
 *   HNET_ADV_STEPPED      what hnet_filters_step does for this session with the host-selected window, gate and repeats included.
 * Readings more than 10 s behind a ring's newest are never used (Propagator.h:110-124), whatever the capacity; the initialiser reads those not older
 * than three windows behind the newest (InertialInitializer.cpp:28-38).  A window that reaches further back than the ring is propagated with what is there.
 * Errors (a bad or repeated id, n > max_batch, feed not enabled, unordered readings) change no state. */
typedef struct hnet_init_params { double window_time, imu_thresh, init_height; int32_t wait_for_jerk; } hnet_init_params;
/* defaults: uzhfpv.launch:18-19,66 (init_window_time 1.0, init_imu_thresh 0.5, init_height 0.1), wait_for_jerk 1 (VioManager.cpp:322) */
void hnet_filter_default_init_params(hnet_init_params* p);
/* allocates the rings, imu_capacity readings (56 bytes) per session, 2 .. 1 << 20; once per filters object (HNET_ERR_INVALID_ARG on a second call) */
int  hnet_filters_enable_feed(hnet_filters* f, int imu_capacity);
int  hnet_filters_set_init_params(hnet_filters* f, int id, const hnet_init_params* p);
/* readings imu[imu_off[i] .. imu_off[i + 1]) for session ids[i] (n distinct sessions, any number of them), appended to its ring by one kernel from one
 * upload; no synchronisation.  Times must be finite and not decrease, within the call and against the ring's newest reading (HNET_ERR_INVALID_ARG,
 * nothing appended for any session).  A full ring drops its oldest readings. */
int  hnet_filters_feed_imu(hnet_filters* f, int n, const int32_t* ids, const hnet_imu* imu, const int64_t* imu_off);
int  hnet_filters_initialized(const hnet_filters* f, int id);             /* 1 after set_state or a successful initialisation, 0 before, -1 for a bad id */
/* camera restarted: the next advance initialises again from the ring; the session's image count restarts (hnet_sessions_reset), the state stays readable */
int  hnet_filters_uninitialize(hnet_filters* f, int id);
enum { HNET_ADV_STEPPED = 0, HNET_ADV_WAIT_IMU = 1, HNET_ADV_WAIT_INIT = 2, HNET_ADV_INITIALIZED = 3, HNET_ADV_PROPAGATED = 4, HNET_ADV_NO_FRAME = 5 };
/* status [n] is required.  state_out [n] (written for STEPPED / PROPAGATED / INITIALIZED sessions), net_out [max_iekf_iteration][n][72] (rows of STEPPED
 * sessions; the others are zero) and updates [n] (as hnet_filters_step; 0 unless STEPPED) may be NULL.  hnet_filters_last_priors afterwards describes the
 * STEPPED sessions, in the order listed. */
int  hnet_filters_advance(hnet_filters* f, int n, const int32_t* ids, hnet_filter_state* state_out, float* net_out, int32_t* updates, int32_t* status);
/* the readings the last advance selected for session id, as hnet_ekf::select_imu_readings writes them: up to cap entries to out, their number to count
 * (0 for a session that advance did not propagate) (tests) */
int  hnet_filters_last_selection(hnet_filters* f, int id, hnet_imu* out, int cap, int* count);

/* ---- filters, between frames: the state predicted to a query time from the IMU rings, read-only ---------------------------------------------
 * A filter's state is the state at its last camera frame.  A control loop wants the pose and velocity NOW, 10 - 30 ms later, at IMU rate: the
 * reference node publishes RosVisualizer::visualize_odometry from its IMU callback (ros_subscribe_cuahn.cpp:134), and OpenVINS' fast_state_propagate
 * (Propagator.h:151, commented out in the reference) carried the state on to the newest reading for it.  hnet_filters_predict does that for the listed
 * sessions from the readings hnet_filters_feed_imu left on the device: the mean of hnet_ekf::propagate_mean_with_imu (the loop of an advance without the
 * covariance) from the state's time to t_query[i] (camera clock), then what the reference's two publishers form from a state
 * (hnet_ekf::odometry_from_state) and the pixel prior a forward at t_query would receive.  p, q, v and prior_px are, bit for bit, what an advance to a
 * frame stamped t_query computes before its forward (tests/test_gpu_filters_predict.py).  The covariance is not predicted here: hnet_filters_predict_cov below returns it.
 * One upload, one launch, one download and one synchronisation on the context's stream, so the call is ordered behind earlier feed_imu / advance calls.
 * No call changes any state: filter states, rings, image counts, mask sequence numbers, hnet_filters_last_timing / _last_selection / _last_priors and
 * the steps so far are as before; sessions with any number of images may be listed.  Per listed session:
 *   HNET_PRED_NO_STATE  the session is not initialised (hnet_filters_initialized).  The record is zero apart from the status.
 *   HNET_PRED_AT_STATE  t_query <= the state's t: the record describes the state as it is, at the state's time, with 0 intervals (no reading is needed
 *                       for that, so this is tested before WAIT_IMU).
 *   HNET_PRED_WAIT_IMU  the newest reading's t - cam_imu_dt <= t_query (the rule of VioManager.cpp:148-149 and of HNET_ADV_WAIT_IMU: the selection closes
 *                       a window only with a reading beyond it).  The record is zero apart from the status.  For the furthest prediction ask just
 *                       below hnet_filters_newest_imu_time(id) - cam_imu_dt.
 *   HNET_PRED_OK        predicted to t_query.  A window that reaches further back than the ring is propagated with what is there, as in the advance.
 * Errors (a bad or repeated id, n > max_batch, feed not enabled, a t_query that is not finite) write nothing.  The first call allocates the call's own
 * scratch (as large as the advance's selection buffer). */
typedef struct hnet_odometry {
    double t_cam, t_imu;            /* the query time (AT_STATE: the state's); + cam_imu_dt, the stamp of the reference's messages */
    double p[3], q[4], v[3];        /* the predicted mean, hnet_filter_state layout */
    double w_pos[3];                /* Rot() * p (publish_state, RosVisualizer.cpp:171) */
    double rpy[3], body_pos[3], body_vel[3];   /* visualize_odometry (RosVisualizer.cpp:121-144): roll / pitch / yaw, front-right-down position and velocity */
    double prior_px[8];             /* what a forward at t_cam would receive as its prior (offsets x 159.5, VioManager.cpp:230-234) */
    int32_t intervals, status;      /* IMU intervals integrated; HNET_PRED_* */
} hnet_odometry;
enum { HNET_PRED_OK = 0, HNET_PRED_NO_STATE = 1, HNET_PRED_WAIT_IMU = 2, HNET_PRED_AT_STATE = 3 };
int    hnet_filters_predict(hnet_filters* f, int n, const int32_t* ids, const double* t_query, hnet_odometry* out);
double hnet_filters_newest_imu_time(const hnet_filters* f, int id);   /* the host mirror's value (IMU clock); NaN: empty ring, feed not enabled or bad id */
/* tools: the launch of the last timed predict, HIP events, ms.  A predict records no events until this has been called once, so a caller at IMU rate
 * never pays for them; the first call switches the timing on and returns NaN, as does every call before a timed predict */
double hnet_filters_last_predict_device_ms(hnet_filters* f);

/* ---- filters, between frames: the predict's record WITH the covariance at the query time, read-only ------------------------------------------
 * hnet_filters_predict gives no uncertainty, and an advance is no substitute for a caller who wants one between frames: it needs a pushed frame,
 * changes the filter, resets the offset block and costs a forward.  hnet_filters_predict_cov returns, for the listed sessions, out[i] = what
 * hnet_filters_predict returns for the same query, byte for byte, and in cov_out[i] the covariance of that record: the 27 x 27 covariance of
 * hnet_ekf::propagate_with_imu at t_query[i], BEFORE any reset (for HNET_PRED_OK bit for bit what the advance to a frame stamped t_query computes before
 * its forward: rows and columns 0 .. 14 are those of its state_out, tests/test_gpu_filters_predict_cov.py), carried to the record's quantities by
 * hnet_ekf::odometry_cov_from_state.  The error state perturbs the attitude on the right (q <- q (x) dq(dtheta)) and p in the IMU frame, so with
 * R = Rot() and P6 = cov[0:6, 0:6]:
 *   pose_cov      J P6 J^T, J = [[R, -R skew(p)], [0, R]]: the covariance of (w_pos, rotation vector about the fixed axes of the frame `global`) in the
 *                 order of a geometry_msgs::PoseWithCovariance (x, y, z, rotation about x, y, z), which publish_state leaves empty (RosVisualizer.cpp:161-176)
 *   body_pos_cov  of body_pos: the signed permutation (-y, -x, -z) applied to pose_cov[0:3, 0:3]
 *   body_vel_cov  of body_vel: the same permutation applied to cov[6:9, 6:9]
 *   prior_cov_px  of prior_px: 159.5^2 cov[sel(i)][sel(j)], sel(j) = 15 + 3 (j >> 1) + (j & 1): the filter's part of the S an update at t_query would form
 *                 (hnet_innovation.s_diag minus the network's share), in px^2
 * There is no roll / pitch / yaw covariance (the Euler Jacobian is singular where Rot2Euler branches); pose_cov[3:6, 3:6] is the attitude's.
 * full_cov: NULL, or [n][729]: the propagated covariance itself, row major in the error-state order of hnet_filter_state.cov (5.8 KB per session, so
 * it is downloaded only when asked for).  Statuses as hnet_filters_predict, decided by the same rules in the same order:
 *   HNET_PRED_OK        the covariance at t_query        HNET_PRED_AT_STATE  the state's covariance as it is, and its blocks
 *   HNET_PRED_NO_STATE / HNET_PRED_WAIT_IMU  zero records and a zero row of full_cov
 * Errors (those of hnet_filters_predict, and a NULL out / cov_out) write nothing.  One upload, one launch, one download and one synchronisation on the
 * context's stream; nothing of the filters' or the sessions' state or bookkeeping is written.  The first call allocates its own job / output block and
 * shares the predict's scratch. */
typedef struct hnet_odometry_cov { double pose_cov[36], body_pos_cov[9], body_vel_cov[9], prior_cov_px[64]; } hnet_odometry_cov;   /* 118 doubles */
int    hnet_filters_predict_cov(hnet_filters* f, int n, const int32_t* ids, const double* t_query, hnet_odometry* out, hnet_odometry_cov* cov_out,
                                double* full_cov);
/* tools: as hnet_filters_last_predict_device_ms, for the launch of the last timed predict_cov */
double hnet_filters_last_predict_cov_device_ms(hnet_filters* f);

/* ---- filters, innovation records: how well each measurement agreed with the filter, and an opt-in gate on it --------------------------------
 * The update weighs the network's covariance with one hand-set scale, k_net_cov, and the reference applies every measurement (it dropped OpenVINS'
 * chi-squared test, UpdaterHNet.cpp:28-61).  With innovations enabled every step / advance also returns, per IEKF iteration and stepping session, the
 * innovation r = mean / 159.5 - prior, the diagonal of S = H P H^T + k_net_cov C / 159.5^2 and the normalised innovation squared NIS = r^T S^-1 r
 * (hnet_ekf::innovation), formed on the device from the state each update is about to change: one more launch per iteration, the records in the call's
 * download, still one upload, one download and one synchronisation.  For a consistent filter the NIS is chi-squared with 8 degrees of freedom: mean 8,
 * quantiles 15.507 (95 %), 20.090 (99 %), 26.124 (99.9 %).
 * The gate (hnet_filters_set_nis_gate; off by default) follows hnet_ekf::iterated_update_gated: at an iteration whose reference gate is open and
 * whose NIS exceeds max_nis, that update and all later updates of the step are skipped for that session; updates already applied stay, every forward
 * still runs (the sequence number advances as always) and the offsets are reset.  A NaN NIS does not reject.  updates[i] keeps its meaning (the number
 * applied, -1 - applied for a singular S): a rejection shows in the records only.  Flags per (iteration, session):
 *   HNET_INNOV_NONE      the reference's gate was closed (VioManager.cpp:257).  r, s_diag and nis are zero.
 *   HNET_INNOV_USED      the update was applied.
 *   HNET_INNOV_REJECTED  the NIS exceeded the session's gate.
 *   HNET_INNOV_SINGULAR  S was singular (nis is NaN).
 *   HNET_INNOV_SKIPPED   after an earlier rejection or singular S in the same step, or a photometric rejection at this or an earlier iteration
 *                        (hnet_filters_set_photo_gate).  r, s_diag and nis are zero.
 * Without hnet_filters_enable_innovations a step and an advance launch exactly what they launched before, and with it and no gate set they compute
 * the same states, priors, network outputs and updates, bit for bit. */
typedef struct hnet_innovation { double r[8], s_diag[8], nis; int32_t iteration, flag; } hnet_innovation;
enum { HNET_INNOV_NONE = 0, HNET_INNOV_USED = 1, HNET_INNOV_REJECTED = 2, HNET_INNOV_SINGULAR = 3, HNET_INNOV_SKIPPED = 4 };
/* per session, accumulated on the host from the records of every accepted step (a repeated attempt never counts twice): records by flag, the sum
 * of the NIS over the USED records (sum_nis / used estimates the mean NIS of what the filter absorbed) and the largest NIS seen, USED or REJECTED */
typedef struct hnet_innovation_stats { int64_t used, rejected, singular; double sum_nis, max_nis; } hnet_innovation_stats;
/* once per filters object (HNET_ERR_INVALID_ARG on a second call): room for [max_iekf_iteration][max_batch] records in the step's output block.
 * hnet_filters_last_priors has nothing to describe until the next step. */
int  hnet_filters_enable_innovations(hnet_filters* f);
/* session id's gate: max_nis = 0 is off (the default), e.g. 20.090 rejects what a consistent filter produces once in 100 frames.  A negative or NaN
 * max_nis, a bad id or a call before hnet_filters_enable_innovations: HNET_ERR_INVALID_ARG */
int  hnet_filters_set_nis_gate(hnet_filters* f, int id, double max_nis);
/* the records [max_iekf_iteration][n] of the last step (n: its n) or advance (n: its STEPPED sessions, in the order listed), as hnet_filters_last_priors.
 * A wrong n, or a last call that ran with innovations off: HNET_ERR_INVALID_ARG, nothing written */
int  hnet_filters_last_innovations(const hnet_filters* f, int n, hnet_innovation* out);
int  hnet_filters_innovation_stats(const hnet_filters* f, int id, hnet_innovation_stats* out);
int  hnet_filters_reset_innovation_stats(hnet_filters* f, int id);

/* ---- photometric residual records: how well a homography agreed with the IMAGES -------------------------------------------------------------
 * The reference's instrument is the error map |warp(img2, H_total) - img1| * 255 (model_to_trace.py:319-327); what an operator of many cameras reads
 * is its mean.  A record is that map summed on the device (csrc/kernels_photo.hip) for H = (float) dlt_solve(p4 + offsets), offsets being 8 floats in
 * pixels, ul, bl, br, ur: for the network's packed mean this is the reference's H_total up to scale.  Every pixel's value has the bits of the err_map
 * paths for the same H; the sums are taken in double in a fixed order (a record depends on its pair and offsets alone, never on the batch or the run).
 * A pixel is "inside" when its sampling position (ix, iy) in img2 has -0.5 < ix < 319.5 and -0.5 < iy < 223.5; sum_inside / n_inside is the residual
 * to watch, because `sum` also holds the pixels that merely left the image (zeros padding).  "estimate << prior ~ identity" means the network is
 * working; "estimate ~ identity" on a moving camera means its output has gone bad, which a consistent NIS cannot show.  No emit_error_map needed. */
typedef struct hnet_photo_residual {
    double  sum;          /* sum over all 71 680 pixels of e = |warp(img2, H)(u, v) - img1(u, v)| * 255, zeros padding: the reference's map, summed */
    double  sum_inside;   /* sum of e over the pixels whose sampling position lies inside img2 */
    int32_t n_inside;     /* their number */
    int32_t flags;        /* HNET_PHOTO_DEGENERATE: H has a non-finite entry (every sample is 0, n_inside = 0); HNET_PHOTO_REJECTED: the session's
                           * photometric gate refused this estimate (a filters step only, hnet_filters_set_photo_gate) */
} hnet_photo_residual;
enum { HNET_PHOTO_DEGENERATE = 1, HNET_PHOTO_REJECTED = 2 };
enum { HNET_PHOTO_MAX_CANDIDATES = 66 };
/* operator call, host pointers: img1 / img2 u8 [n][224][320], offsets_px [n][m][8], out [n][m]; map_out NULL or float [n][m][224][320] (the map itself).
 * 1 <= n <= max_batch, 1 <= m <= 66 (HNET_ERR_CAPACITY / HNET_ERR_INVALID_ARG otherwise; an error writes nothing).  One upload, one download, one
 * synchronisation on the context's stream. */
int  hnet_op_photo_residual(hnet_ctx* ctx, const uint8_t* img1, const uint8_t* img2, int n, const float* offsets_px, int m, hnet_photo_residual* out,
                            float* map_out);
/* the same on the current pair of each listed session (img1 / img2 = the frames a forward receives as prev / curr), for any hypothesis, e.g.
 * hnet_odometry.prior_px of a predict at the frame's time.  Read-only: counts, sequence numbers, times and hnet_sessions_last_timing stay as they were.
 * Errors as hnet_sessions_infer: a bad or repeated id (HNET_ERR_INVALID_ARG), fewer than two images (HNET_ERR_NOT_READY), n > max_batch (HNET_ERR_CAPACITY) */
int  hnet_sessions_photo_residual(hnet_sessions* s, int n, const int32_t* ids, const float* offsets_px, int m, hnet_photo_residual* out);
/* once per filters object (HNET_ERR_INVALID_ARG on a second call; works with hnet_filters_enable_innovations in either order): from now on every step
 * and advance also produces, per stepping session, 2 + max_iekf_iteration records on the step's own frame pair - [0] zero offsets (no motion), [1] the
 * fp32 prior of iteration 0 (what hnet_filters_last_priors reports, whether or not use_prior let the forward read it), [2 + it] the packed mean of
 * forward `it` - inside the call's one download, two launches after the last update.  Unless a photometric gate is set (hnet_filters_set_photo_gate,
 * below) nothing is gated on them, and the states, priors, network outputs, updates, innovation records and sequence numbers are what they are
 * without the call, bit for bit.  hnet_filters_last_priors has nothing to describe until the next step. */
int  hnet_filters_enable_photometric(hnet_filters* f);
/* the records [n][2 + max_iekf_iteration] of the last step (n: its n) or advance (n: its STEPPED sessions, in the order listed).  A wrong n, or a last
 * call that ran without hnet_filters_enable_photometric (or in which nothing stepped): HNET_ERR_INVALID_ARG, nothing written */
int  hnet_filters_last_photometric(const hnet_filters* f, int n, hnet_photo_residual* out);
/* The photometric gate, per session and off by default: refuse an update whose estimate explains the frame pair WORSE than the IMU prior did, before it
 * is absorbed.  The rule is hnet_ekf::photo_reject and the loop hnet_ekf::iterated_update_photo_gated (include/hnet_ekf.h): at every iteration whose
 * reference gate is open (VioManager.cpp:257) and that no singular S, NIS rejection or photometric rejection of the step precedes, record [2 + it] is
 * judged against record [1].  Refused: an estimate that is DEGENERATE or has fewer than max(min_inside, 1) pixels inside; otherwise, given a prior record
 * that is not DEGENERATE and has that many pixels inside, an estimate with
 *   est.sum_inside * prior.n_inside > (max_ratio * prior.sum_inside) * est.n_inside          (a NaN on either side does not refuse).
 * A refusal sets HNET_PHOTO_REJECTED in record [2 + it]; that update and all later updates of the step are skipped for that session, updates already
 * applied stay, every forward still runs (the sequence number advances as always), the offsets are reset, updates[i] counts what was applied, and the
 * innovation records from that iteration on are HNET_INNOV_SKIPPED.  The photometric gate comes before the NIS gate: a refused estimate has no NIS.
 * A step or advance in which at least one STEPPING session has a gate forms the records per iteration, between the forward and the update they guard
 * (two launches per iteration; img2 is read once per iteration) instead of after the last update, for all its stepping sessions: the records have the
 * same bits either way, and so have the states, outputs and records of the sessions without a gate.  hnet_filters_last_timing's device window then
 * includes the photometric launches, which without a gate lie behind it.  Still one upload, one download and one synchronisation; an overflow or
 * chain-timeout repeat forms every verdict again.
 * max_ratio = 0 is off.  HNET_ERR_INVALID_ARG, nothing changed: a negative or NaN max_ratio, min_inside outside 0 .. 71 680, a bad id, a call before
 * hnet_filters_enable_photometric. */
int  hnet_filters_set_photo_gate(hnet_filters* f, int id, double max_ratio, int32_t min_inside);
/* per session, accumulated on the host from the records of every accepted step or advance with photometric records, gated or not (a repeated attempt
 * never counts twice).  judged: the estimate records [2 + it] of iterations whose reference gate was open and that no singular S, NIS rejection or
 * photometric rejection preceded; rejected, degenerate: those among them with HNET_PHOTO_REJECTED, HNET_PHOTO_DEGENERATE.  sum_ratio, max_ratio: over
 * the judged records for which ratio = (est.sum_inside / est.n_inside) / (prior.sum_inside / prior.n_inside) is defined and finite (neither record
 * DEGENERATE, both n_inside >= 1), in host arithmetic. */
typedef struct hnet_photo_stats { int64_t judged, rejected, degenerate; double sum_ratio, max_ratio; } hnet_photo_stats;
int  hnet_filters_photo_stats(const hnet_filters* f, int id, hnet_photo_stats* out);
int  hnet_filters_reset_photo_stats(hnet_filters* f, int id);
/* tools: where the single-candidate launch of iterations 1 .. of a gated step takes its taps of img2 from: 0 LDS (the pair staged per workgroup), 1 global
 * memory.  The records do not depend on it (tests/test_gpu_filters_photo_gate.py); the default is the one DESIGN 7j measured as faster. */
int  hnet_filters_set_photo_gate_taps(hnet_filters* f, int from_global);

/* ---- photometric alignment: which way a homography is wrong, how strongly the frame pair constrains it, and a better one -----------------------------
 * Forward-additive Lucas-Kanade / Levenberg-Marquardt on the eight corner offsets x (pixels, ul bl br ur), on the device (csrc/kernels_photo_align.hip),
 * minimising the squared form of the residual hnet_photo_residual sums.  The quantity (the shared code is include/hnet_photo_align.h):
 *   H(x) = (float) dlt_solve(p4 + x) as for the records; pixel (u, v) samples img2 at (ix, iy) = (X / Z, Y / Z), the records' exact sampler.
 *   A pixel is VALID when 0 <= ix < 319 and 0 <= iy < 223, so that every one of its four bilinear taps is a pixel of img2.  This is deliberately stricter
 *   than the records' "inside": the zero padding puts a false edge of full contrast around the image, which drags a minimiser away from the truth.
 *   r = (w - img1 / 255) * 255 in grey levels, w the bilinear sample (|r| has the bits of the error map); with taps a b / c d and fractions fx, fy
 *   gx = ((b - a)(1 - fy) + (d - c) fy) * 255, gy = ((c - a)(1 - fx) + (d - b) fx) * 255, q = gx ix + gy iy, and the row of dr / dvec(H) is
 *   s = (gx u, gx v, gx, gy u, gy v, gy, -q u, -q v, -q) / Z.  Over the valid pixels: sum s s^T, sum s r, sum r^2, n_valid, summed in double in a
 *   fixed order (a record depends on its pair, start offsets and options alone, never on the batch or the run).
 *   D = dvec(H) / dx (9 x 8) is the analytic derivative of dlt_solve, in double.  info = A = D^T (sum s s^T) D in grey^2 / px^2, grad = g = D^T (sum s r),
 *   mse = sum r^2 / n_valid.
 * One step (hnet_align::step): dx = -(A + lambda diag(A))^-1 g by Cholesky in double; the trial x + dx (rounded to fp32) is accepted iff it has
 * n_valid >= max(min_valid, 9) and a strictly smaller mse; lambda starts at lambda0, x 0.1 on accept, x 10 on reject.  A pair stops with
 *   HNET_ALIGN_CONVERGED   after an accepted step with max |dx| < eps_px.  The flag reports a small accepted STEP, not a small residual: after a run of
 *                          refusals (accepted << trials, a large lambda) the damping alone makes the step small, so look at mse against mse0 and at lambda
 *                          before reading it as "aligned";
 *   HNET_ALIGN_SINGULAR    when A at offsets_px has a Cholesky pivot <= 1e-12 max diag(A) or a non-finite one: the pair does not constrain all eight
 *                          offsets (a constant img2: A = 0 exactly; stripes).  The offsets stay where they are.  Also reported with max_iterations = 0;
 *   HNET_ALIGN_DEGENERATE  when the start offsets have no homography, HNET_ALIGN_FEW_PIXELS when they have fewer than max(min_valid, 9) valid pixels:
 *                          the start offsets come back unchanged with info = grad = 0 (mse0 = mse = 0).
 * No flag: max_iterations trials were made.  max_iterations = 0 is the linearisation alone (info, grad, mse at offsets0_px).
 * `info` is an INFORMATION matrix, not a calibrated covariance: sigma^2 A^-1 with sigma^2 = mse understates the error of offsets_px severalfold (u8
 * rounding and interpolation error are not white noise).  Its scaling is the caller's.
 * The basin of convergence of this single-level call is the texture scale: start within a pixel or two of the truth on fine texture.  A start that is further
 * off belongs to hnet_op_photo_align_pyramid below, which runs the same alignment coarse to fine over an image pyramid. */
typedef struct hnet_photo_align_opts { int32_t max_iterations;  /* 0 .. 32 */  int32_t min_valid;  double lambda0, eps_px; } hnet_photo_align_opts;
void hnet_photo_align_default_opts(hnet_photo_align_opts* o);      /* 6, 20000, 1e-3, 1e-3 */
typedef struct hnet_photo_align {
    float   offsets_px[8];         /* where the alignment ended (the start offsets for max_iterations = 0 or an early stop) */
    double  mse0, mse;             /* mean squared residual over the valid pixels at the start and at offsets_px, grey levels^2 */
    int32_t n_valid0, n_valid;     /* valid pixels at the start and at offsets_px */
    int32_t trials, accepted;      /* steps tried (linearisations after the first) and accepted: accepted <= trials <= max_iterations */
    int32_t flags;                 /* HNET_ALIGN_* (the alignment gap behind it is written as zero: records compare byte for byte) */
    double  lambda, grad[8], info[64];   /* the damping reached; g and A = J^T J at offsets_px */
} hnet_photo_align;
enum { HNET_ALIGN_CONVERGED = 1, HNET_ALIGN_SINGULAR = 2, HNET_ALIGN_DEGENERATE = 4, HNET_ALIGN_FEW_PIXELS = 8 };
enum { HNET_ALIGN_MAX_ITERATIONS = 32 };
/* operator call, host pointers: img1 / img2 u8 [n][224][320], offsets0_px [n][8], out [n].  1 <= n <= max_batch (HNET_ERR_CAPACITY); a null pointer or
 * options out of range (max_iterations outside 0 .. 32, min_valid < 0, lambda0 <= 0 or > 1e100, eps_px < 0, a non-finite one): HNET_ERR_INVALID_ARG.  lambda0 is
 * capped so that lambda, x 10 per refusal, stays far from overflow (at most 1e132 after 32 refusals): HNET_ALIGN_SINGULAR is never an artefact of the damping.
 * An error writes nothing.  One upload, max_iterations + 1 pairs of launches (iterations are separate launches; a stopped pair's workgroups return at once), one
 * download and one synchronisation on the context's stream. */
int  hnet_op_photo_align(hnet_ctx* ctx, const uint8_t* img1, const uint8_t* img2, int n, const float* offsets0_px, const hnet_photo_align_opts* opts,
                         hnet_photo_align* out);
/* the same on the current pair of each listed session, e.g. from hnet_odometry.prior_px of a predict at the frame's time, or from an estimate the
 * photometric gate refused.  Read-only: counts, sequence numbers, times and hnet_sessions_last_timing stay as they were.  Errors as
 * hnet_sessions_photo_residual. */
int  hnet_sessions_photo_align(hnet_sessions* s, int n, const int32_t* ids, const float* offsets0_px, const hnet_photo_align_opts* opts, hnet_photo_align* out);
/* device time of the launch sequence of the context's last alignment call (HIP events of its own around it), milliseconds */
double hnet_last_photo_align_device_ms(hnet_ctx* ctx);

/* ---- coarse-to-fine photometric alignment over a device image pyramid (csrc/kernels_photo_pyramid.hip; the shared code is include/hnet_photo_pyramid.h) ----
 * Levels 1, 2, 3 of a frame are 160 x 112, 80 x 56 and 40 x 28 u8, each the 2 x 2 box mean of the level below, (a + b + c + d + 2) >> 2, cascaded (exact
 * integers).  A call with `levels` in 1 .. 4 runs ONE COMPLETE alignment per level, from level levels - 1 down to level 0, each from the offsets at which the
 * level above ended (the coarsest from offsets0_px), WHATEVER that level's flags: a flag stops its own level only.  The offsets, grad, info and the steps stay
 * in full-resolution pixels at every level; level-L pixel (u, v) stands at (2^L u + c, 2^L v + c), c = (2^L - 1) / 2, is VALID when all four taps are pixels
 * of the level-L img2, and its gradient is taken per full-resolution pixel.  The options are the call's, max_iterations PER LEVEL and min_valid >> 2 L at
 * level L (still floored at 9).  levels = 1 is hnet_op_photo_align, byte for byte.  With 4 levels and 8 trials per level the repository's stock texture is
 * aligned from zero offsets when the truth is up to 32 px away, where the single-level call needs a start within about 1.5 px.
 * out [n]: the level-0 records.  levels_out: NULL or [n][levels], index = level: the complete record of every level, its mse in grey^2 of that level's
 * images and its n_valid* counting that level's pixels.  A start without a homography is DEGENERATE at every level, a constant img2 SINGULAR at every level
 * with the offsets unchanged, a far-out start FEW_PIXELS at every level.
 * Errors are those of hnet_op_photo_align, and levels outside 1 .. 4: HNET_ERR_INVALID_ARG.  An error writes nothing.  One upload, one pyramid launch, per
 * level a gather of the start offsets and max_iterations + 1 pairs of launches, one download and one synchronisation; hnet_last_photo_align_device_ms covers
 * the whole sequence.  The pyramid's device scratch (2 x max_batch x 23 520 bytes) is allocated by the context's first such call. */
enum { HNET_ALIGN_MAX_LEVELS = 4 };
int  hnet_op_photo_align_pyramid(hnet_ctx* ctx, const uint8_t* img1, const uint8_t* img2, int n, const float* offsets0_px, const hnet_photo_align_opts* opts,
                                 int levels, hnet_photo_align* out /* [n] */, hnet_photo_align* levels_out /* NULL or [n][levels], index = level */);
/* the same on the current pair of each listed session; read-only like hnet_sessions_photo_align, errors as there plus `levels` */
int  hnet_sessions_photo_align_pyramid(hnet_sessions* s, int n, const int32_t* ids, const float* offsets0_px, const hnet_photo_align_opts* opts, int levels,
                                       hnet_photo_align* out, hnet_photo_align* levels_out);
/* operator level (tests): levels 1 .. 3 of n host frames u8 [n][224][320] -> out [n][17920 + 4480 + 1120] bytes, level 1 first.  1 <= n <= max_batch */
int  hnet_op_photo_pyramid(hnet_ctx* ctx, const uint8_t* img, int n, uint8_t* out);

/* ---- photometric alignment with a gain / bias model and Huber weights (csrc/kernels_photo_robust.hip; the shared code is include/hnet_photo_robust.h) ----
 * The coarse-to-fine call above on TEN parameters: the eight offsets, a gain G and a bias b (grey levels) applied to the sampled img2, for frames of an
 * auto-exposure camera, and a Huber loss for pixels no homography explains.  Per valid pixel r = ((float) G w + (float)(b / 255) - img1 / 255) * 255; with
 * k = huber_k (grey levels; 0: quadratic) a pixel with |r| <= k costs rho = r^2 and weighs omega = 1, any other costs rho = k (2 |r| - k) and weighs
 * omega = k / |r| (an OUTLIER).  The loop is the same Levenberg-Marquardt descent, on the mean of rho (a fixed function of the ten parameters, not a
 * re-weighted least squares on a moving target): a trial is accepted iff it has a homography, a finite positive gain, a finite bias, at least
 * max(min_valid, 9) valid pixels and a strictly smaller mean rho.  HNET_ALIGN_CONVERGED is judged on the eight offset components of the step alone;
 * HNET_ALIGN_SINGULAR on the undamped 10 x 10 (8 x 8 with the model off) matrix.  Levels, min_valid >> 2 L, the start of a level (gain and bias are carried
 * like the offsets) and the flags are hnet_op_photo_align_pyramid's.
 * brightness = 0 keeps G = 1, b = 0 and solves the 8 x 8 system; with huber_k = 0 besides, the field `px` of every record of every level equals
 * hnet_op_photo_align_pyramid's record byte for byte.
 * px.mse0 / px.mse are the mean rho, px.grad / px.info the offset block of grad10 / info10 at the record's gain.  grad10 / info10: the gradient and the
 * Gauss-Newton matrix in (offsets [8], gain, bias); rows and columns 8, 9 are zero when the model is off.  n_outliers0 / n_outliers: the valid pixels with
 * omega < 1 at the start / at the record's point.  Saturated pixels break the affine model and are left to the Huber weights.
 * Errors are those of hnet_op_photo_align_pyramid, and HNET_ERR_INVALID_ARG for brightness outside 0 / 1, a negative or non-finite huber_k, a non-finite or
 * non-positive gain0, a non-finite bias0, or gain0 != 1 / bias0 != 0 with the model off.  An error writes nothing.  One upload, the launch sequence, one
 * download of the records and one synchronisation; hnet_last_photo_align_device_ms covers the whole sequence. */
typedef struct hnet_photo_robust_opts {
    hnet_photo_align_opts base;
    int32_t brightness;        /* 0 off, 1 gain + bias */
    int32_t pad;
    double  huber_k;           /* grey levels, 0 = quadratic */
    double  gain0, bias0;      /* start, 1 and 0 */
} hnet_photo_robust_opts;
typedef struct hnet_photo_robust {
    hnet_photo_align px;       /* common fields: mse0 / mse are the mean robust cost; grad / info are the offset block at the current gain */
    double  gain, bias;
    int32_t n_outliers0, n_outliers;
    double  grad10[10], info10[100];   /* zero rows / columns 8, 9 when the model is off */
} hnet_photo_robust;
void hnet_photo_robust_default_opts(hnet_photo_robust_opts* o);      /* base defaults, 1, 10.0, 1, 0 */
int  hnet_op_photo_align_robust(hnet_ctx* ctx, const uint8_t* img1, const uint8_t* img2, int n, const float* offsets0_px, const hnet_photo_robust_opts* opts,
                                int levels, hnet_photo_robust* out /* [n] */, hnet_photo_robust* levels_out /* NULL or [n][levels], index = level */);
/* the same on the current pair of each listed session; read-only like hnet_sessions_photo_align_pyramid */
int  hnet_sessions_photo_align_robust(hnet_sessions* s, int n, const int32_t* ids, const float* offsets0_px, const hnet_photo_robust_opts* opts, int levels,
                                      hnet_photo_robust* out, hnet_photo_robust* levels_out);
/* hnet_op_photo_align_robust on the template pixels a mask admits (include/hnet_photo_masked.h).  mask1: u8 [n][224][320] beside img1;
 * non-zero: the pixel takes part.  Level L of the mask is 1 where all 4^L level-0 bytes under a pixel are non-zero (an AND), so a coarse template pixel whose
 * box mean mixes admitted and refused bytes is never used.  A refused pixel adds nothing to any sum, to n_valid or to n_outliers; img1 under it is never
 * read into a sum.  Options, levels, the per-level min_valid (NOT scaled by the mask: a mask that admits too little stops HNET_ALIGN_FEW_PIXELS), records and
 * flags are the robust call's; a mask without a zero byte gives its records byte for byte.  Errors are those of hnet_op_photo_align_robust, and
 * HNET_ERR_INVALID_ARG for a null mask.  One upload {img1 | mask1 | img2 | offsets}, the mask pyramid and the launch sequence, one download, one
 * synchronisation; hnet_last_photo_align_device_ms covers the mask pyramid and the sequence. */
int  hnet_op_photo_align_masked(hnet_ctx* ctx, const uint8_t* img1, const uint8_t* mask1, const uint8_t* img2, int n, const float* offsets0_px,
                                const hnet_photo_robust_opts* opts, int levels, hnet_photo_robust* out /* [n] */,
                                hnet_photo_robust* levels_out /* NULL or [n][levels], index = level */);
/* host only: the information matrix and gradient of the offsets with gain and bias marginalised (the Schur complement of the 2 x 2 brightness block of
 * info10): what a filter may use when brightness is a nuisance.  With the model off (rows 8, 9 of info10 all zero) it copies px.info / px.grad.
 * HNET_ERR_INVALID_ARG, nothing written, for a null argument or when the 2 x 2 block has no Cholesky factor. */
int  hnet_photo_robust_marginal(const hnet_photo_robust* rec, double info8[64], double grad8[8]);

/* ---- hnet_filters: a photometric alignment as the fallback measurement after a refusal (csrc/kernels_filters_refine.hip; the shared code is
 * include/hnet_photo_refine.h).  Per session and off by default.  When the photometric gate (hnet_filters_set_photo_gate) refuses a session's
 * estimate at ITERATION 0, the session would get no measurement this frame.  With refinement on, the step instead runs hnet_op_photo_align_robust's
 * launch sequence on the session's frame pair from iteration 0's fp32 prior (hnet_filters_last_priors row 0) and applies the level-0 record as the
 * measurement of one more update, hnet_ekf::iterated_update_photo_refined:
 *   mean  = px.offsets_px,
 *   R_px  = cov_scale * px.mse * inverse(info8) + sigma_floor_px^2 I, symmetrised, info8 = hnet_photo_robust_marginal's,
 * handed to the unchanged update as the packed record {mean | (float)(R_px / k_net_cov)}, against the prior of the propagated state, with
 * update_offset = 0; the offsets are reset afterwards as always.  cov_scale is the CALLER's: nothing calibrates mse * inverse(info8) against the real
 * error (correlated pixels make it too small; tools/photo_refine_calibrate.py prints what synthetic texture says) - hence no default.
 * The measurement is UNUSABLE, and the session keeps the state the refusal alone leaves, when (one reason bit each, tested in this order) k_net_cov is not
 * finite and positive; the record stopped HNET_ALIGN_SINGULAR, _DEGENERATE or _FEW_PIXELS; no trial was accepted at any level (the "measurement" would be
 * the prior itself); max_mse > 0 and px.mse > max_mse; the marginal has no Cholesky factor (a pivot <= 1e-12 max diag) or the inverse reports singular;
 * an entry of R_px is not finite.
 * updates[i] counts the fallback update when it is applied; a fallback S found singular is reported as the existing -1 - applied (= -1).  The records of
 * hnet_filters_last_innovations and hnet_filters_last_photometric keep their shape and content; the fallback's innovation lives in the refine record
 * (iteration = max_iekf_iteration) and is filled whether or not hnet_filters_enable_innovations was called.  The session's NIS gate, when set, applies to
 * the fallback.  A refusal at iteration >= 1, a NIS rejection and a singular S trigger no fallback.
 * A step or advance in which at least one STEPPING session has refinement on AND a photometric gate enqueues the fallback's launches for all its
 * stepping sessions (the host knows the configuration, never the verdicts; sessions not refused align from NaN offsets, which costs their workgroups an
 * early return): 3 small kernels, the alignment's sequence, one prior, one innovation and one update launch, inside the attempt (a repeat redoes
 * them) and inside hnet_filters_last_timing's device window.  Still one upload, one download, one synchronisation.  Any other call launches exactly what
 * it launched before, and its results are bit for bit what they are without this API.  All refining sessions of one call must share `align` and `levels`
 * (one launch sequence serves them): a mismatch is HNET_ERR_INVALID_ARG from the step or advance, nothing changed; cov_scale, sigma_floor_px and max_mse
 * are per session. */
typedef struct hnet_photo_refine_opts {
    hnet_photo_robust_opts align;
    int32_t levels;            /* 1 .. 4 */
    int32_t pad;
    double  cov_scale;         /* > 0; hnet_photo_refine_default_opts leaves 0 on purpose: the caller must choose it */
    double  sigma_floor_px;    /* >= 0: sigma_floor_px^2 is added to the diagonal of R_px */
    double  max_mse;           /* 0 = no limit; else a record with px.mse above it is unusable */
} hnet_photo_refine_opts;
void hnet_photo_refine_default_opts(hnet_photo_refine_opts* o);      /* robust defaults, 3, 0 (!), 0.05, 0 */
enum { HNET_REFINE_ASKED = 1,            /* the gate refused iteration 0 of a session with refinement on: `rec` is its alignment's level-0 record */
       HNET_REFINE_APPLIED = 2,          /* the fallback update was applied */
       HNET_REFINE_NIS_REJECTED = 4,     /* the session's NIS gate refused the fallback */
       HNET_REFINE_S_SINGULAR = 8,       /* the fallback's S was singular */
       HNET_REFINE_BAD_K_NET_COV = 16, HNET_REFINE_STOPPED = 32, HNET_REFINE_NO_STEP = 64, HNET_REFINE_MSE_ABOVE_MAX = 128, HNET_REFINE_NO_FACTOR = 256,
       HNET_REFINE_NON_FINITE = 512,     /* the UNUSABLE reasons, in the order above */
       HNET_REFINE_UNUSABLE = 16 | 32 | 64 | 128 | 256 | 512 };
typedef struct hnet_photo_refine {
    hnet_photo_robust rec;     /* level 0 of the alignment: byte for byte hnet_sessions_photo_align_robust's from the same start and options */
    double  r_px[64];          /* zeros when unusable */
    hnet_innovation innov;     /* hnet_ekf::innovation of the fallback measurement; iteration = max_iekf_iteration; HNET_INNOV_NONE (zeros) when unusable */
    int32_t flags;             /* HNET_REFINE_*; 0 (and the whole record zero) for a session that asked for no fallback */
    int32_t pad;               /* written as zero: records compare byte for byte */
} hnet_photo_refine;
/* opts == NULL turns refinement off for the session.  The first call with options allocates the alignment's scratch and grows the output block
 * (hnet_filters_last_* have nothing to describe until the next step).  HNET_ERR_INVALID_ARG, nothing changed: a bad id, a call before
 * hnet_filters_enable_photometric, options hnet_op_photo_align_robust would refuse, levels outside 1 .. 4, cov_scale <= 0 or not finite, a negative or
 * non-finite sigma_floor_px or max_mse. */
int  hnet_filters_set_photo_refine(hnet_filters* f, int id, const hnet_photo_refine_opts* opts);
/* the records [n] of the last step (n: its n) or advance (n: its STEPPED sessions, in the order listed).  A wrong n, or a last call that ran without a
 * refining session: HNET_ERR_INVALID_ARG, nothing written */
int  hnet_filters_last_refine(const hnet_filters* f, int n, hnet_photo_refine* out);
/* per session, accumulated on the host from the records of accepted calls only (a repeated attempt never counts twice): asked, applied, unusable (any
 * reason bit), nis_rejected; sum_nis / max_nis over the fallbacks whose NIS was formed and finite (applied or NIS-rejected): what a caller calibrates
 * cov_scale with (a consistent filter gives a mean of 8). */
typedef struct hnet_refine_stats { int64_t asked, applied, unusable, nis_rejected; double sum_nis, max_nis; } hnet_refine_stats;
int  hnet_filters_refine_stats(const hnet_filters* f, int id, hnet_refine_stats* out);
int  hnet_filters_reset_refine_stats(hnet_filters* f, int id);

/* ---- sessions, keyframes: each camera tracked against a HELD frame, on the device (csrc/kernels_keyframe.hip; the shared code is include/hnet_keyframe.h;
 * DESIGN 7p).  Opt-in: a sessions object that never calls hnet_sessions_enable_keyframes allocates, launches and returns exactly what it did before.
 * Everything else in this header measures between two consecutive frames, so a camera that hovers integrates frame-to-frame homographies and drifts
 * without bound.  Here every session holds a KEYFRAME longer than one tick, and one call aligns the session's current frame against it with
 * hnet_op_photo_align_robust's launch sequence: a measurement whose error does not grow with the number of frames.
 * Conventions: offsets x are ul, bl, br, ur in pixels, H(x) = dlt_solve(p4 + x) in double with h[8] = 1 maps a template pixel to its sampling position in
 * the other image, hence H_key->curr = H_prev->curr . H_key->prev.  Per session the device keeps {has_key, key_px (key -> previous tracked frame),
 * h_origin_key (origin -> keyframe; the origin is the first keyframe since the last reset), age, keyframes}.
 * One track, per listed session:
 *   no keyframe yet: curr becomes the keyframe, HNET_KF_FIRST | HNET_KF_REKEYED, h_origin_curr = I, keyframes = 1, everything else zero.
 *   else start_px = the corners of H(step_px) . H(key_px) minus p4 (step_px: the caller's prev -> curr offsets, e.g. the network's mean; NULL = no
 *     motion); the alignment key -> curr runs from it and `rec` is its level-0 record, byte for byte hnet_op_photo_align_robust(keyframe, curr,
 *     start_px) with the same options.  A start without a homography is quiet NaNs, on which the alignment reports HNET_ALIGN_DEGENERATE.
 *   LOST (one reason bit, in this order): HNET_KF_NO_START; HNET_KF_STOPPED (rec stopped SINGULAR, DEGENERATE or FEW_PIXELS); HNET_KF_MSE_ABOVE_MAX
 *     (max_mse > 0 and not mse <= max_mse); HNET_KF_NON_FINITE (an offset of rec).  A start that accepted no trial is not lost.  With auto_rekey the
 *     session re-keys on curr (HNET_KF_REKEYED | HNET_KF_BRIDGED) and the origin chain is extended by the composed start (by the previous key_px when
 *     the start has no homography): dead reckoning.  Without it the keyframe stays and key_px becomes the start (HNET_KF_BRIDGED) when that has a
 *     homography.
 *   TRACKED (all else): key_px = rec's offsets.  With auto_rekey the session re-keys AFTER this frame when overlap < rekey_overlap
 *     (HNET_KF_LOW_OVERLAP) or max_age > 0 and age >= max_age (HNET_KF_MAX_AGE).
 *   In both: age + 1, overlap = rec.px.n_valid / 71 680, h_origin_curr = H(key_px) . h_origin_key renormalised to h[8] = 1.  A re-key makes curr the
 *   keyframe: h_origin_key = h_origin_curr, key_px = 0, age = 0, keyframes + 1.  The record's key_px and age are the frame's against the keyframe it was
 *   measured on; keyframes counts the new one.  When a product of the origin chain has a non-finite entry or |h[8]| below 1e-12 of its largest entry
 *   the chain restarts at the current keyframe (HNET_KF_ORIGIN_RESTARTED).  HNET_KF_GAP: the session's image count is not its count at the previous track + 1
 *   (frames no track saw, or the same frame tracked again); it changes nothing else (the alignment's basin, 32 px at 3 levels, decides whether the start served).
 * hnet_sessions_keyframe_track is read-only for everything the sessions had before: counts, ring, stamps, sequence numbers and
 * hnet_sessions_last_timing stay as they were (it uses the context's staging arrays like hnet_sessions_photo_align_robust).
 * Errors, nothing changed and nothing written: HNET_ERR_INVALID_ARG for a call before hnet_sessions_enable_keyframes, a second enable, a null opts or
 * out, options hnet_op_photo_align_robust would refuse, levels outside 1 .. 4, auto_rekey outside 0 / 1, max_age < 0, rekey_overlap outside 0 .. 1, a
 * negative or non-finite max_mse, n < 1, an id out of range or repeated; HNET_ERR_CAPACITY for n > max_batch; HNET_ERR_NOT_READY for a listed session
 * without an image.
 * Enable allocates the keyframe store [n_sessions][71 680] bytes (zeroed), the state table and the alignment's scratch for max_batch.  A track is ONE
 * upload {step | ids | curr slot | gap}, 4 small launches around the alignment's sequence (start, gather, decide, commit), ONE download of the records [n]
 * and one synchronisation; hnet_sessions_last_keyframe_device_ms covers the launches (events of its own). */
typedef struct hnet_keyframe_opts {
    hnet_photo_robust_opts align;
    int32_t levels;            /* 1 .. 4 */
    int32_t auto_rekey;        /* 0 / 1 */
    int32_t max_age;           /* >= 0; 0 = no limit */
    int32_t pad;
    double  rekey_overlap;     /* 0 .. 1 */
    double  max_mse;           /* >= 0; 0 = no limit */
} hnet_keyframe_opts;
enum { HNET_KF_FIRST = 1, HNET_KF_REKEYED = 2, HNET_KF_BRIDGED = 4, HNET_KF_GAP = 8,
       HNET_KF_LOW_OVERLAP = 16, HNET_KF_MAX_AGE = 32,                                                   /* the re-key reasons of a TRACKED frame */
       HNET_KF_NO_START = 64, HNET_KF_STOPPED = 128, HNET_KF_MSE_ABOVE_MAX = 256, HNET_KF_NON_FINITE = 512,    /* the LOST reasons, in the order tested */
       HNET_KF_ORIGIN_RESTARTED = 1024,
       HNET_KF_LOST = 64 | 128 | 256 | 512 };
typedef struct hnet_keyframe_track {
    hnet_photo_robust rec;      /* level 0, key -> curr; zeros when no alignment result was read (HNET_KF_FIRST) */
    float   start_px[8];        /* what the alignment started from (quiet NaNs: no homography) */
    float   key_px[8];          /* key -> curr: rec's offsets when TRACKED, the bridge when LOST */
    double  h_origin_curr[9];   /* origin -> curr, h[8] = 1 */
    double  overlap;            /* rec.px.n_valid / 71 680 */
    int32_t age;                /* frames tracked on the keyframe this one was measured on, this one included */
    int32_t keyframes;          /* keyframes taken since the last reset, a re-key of this frame included */
    int32_t flags;              /* HNET_KF_* */
    int32_t pad;                /* written zero: records compare byte for byte */
} hnet_keyframe_track;
void hnet_keyframe_default_opts(hnet_keyframe_opts* o);      /* robust defaults, levels 3, auto_rekey 1, max_age 0, rekey_overlap 0.6, max_mse 0 */
int  hnet_sessions_enable_keyframes(hnet_sessions* s);       /* once; a second call is HNET_ERR_INVALID_ARG */
int  hnet_sessions_keyframe_track(hnet_sessions* s, int n, const int32_t* ids, const float* step_px /* [n][8] prev -> curr, or NULL = no motion */,
                                  const hnet_keyframe_opts* opts, hnet_keyframe_track* out /* [n] */);
/* drops the session's keyframe and origin chain: its next track is HNET_KF_FIRST.  hnet_sessions_reset does the same when keyframes are enabled.
 * Stream ordered, no synchronisation.  HNET_ERR_INVALID_ARG before enable or for an id out of range. */
int  hnet_sessions_keyframe_reset(hnet_sessions* s, int id);
/* operator level (tests): the session's keyframe, 224 x 320 bytes; HNET_ERR_NOT_READY without one.  One download, one synchronisation. */
int  hnet_sessions_get_keyframe(hnet_sessions* s, int id, uint8_t* out);
double hnet_sessions_last_keyframe_device_ms(hnet_sessions* s);     /* 0 before the first track; of the last track, revisit or relocalise */

/* ---- sessions, a MAP of keyframes and closing loops against it, on the device (csrc/kernels_keyframe_map.hip; the shared code is
 * include/hnet_keyframe_map.h).  Opt-in on top of the keyframes: a sessions object that never calls hnet_sessions_enable_keyframe_map allocates,
 * launches and returns exactly what it did before, and with a map the track's records stay byte for byte what they are without one.
 * A track removes the drift of a camera that stays on one keyframe, not the drift of the keyframe chain: every re-key extends h_origin_key by one
 * measured link, a lost frame by dead reckoning, and the old keyframe is overwritten.  With a map every keyframe a track takes is also kept in one of
 * `capacity` (2 .. 8) slots per session, as {valid, links, serial, h_origin_key}: links counts the chain links between the origin and that keyframe,
 * serial numbers the session's stored keyframes from 1.  Slot 0 is never evicted (the oldest keyframe the chain knows), slots 1 .. capacity-1 are a
 * ring.  HNET_KF_ORIGIN_RESTARTED and HNET_KF_FIRST invalidate the session's entries; hnet_sessions_keyframe_reset and hnet_sessions_reset clear them.
 * One revisit, per listed session (its latest image must be the one its last track saw: the state's key_px then describes the current frame):
 *   h_origin_before = H(key_px) . h_origin_key, the chain's value for the current frame.  For every valid entry other than the current keyframe's with
 *   FEWER links than it, G = h_origin_before . inverse(entry.h_origin_key) predicts where the stored keyframe lies in the current frame; of an inset
 *   8 x 8 grid of its pixels (20 + 40 i, 14 + 28 j) `grid` lie inside the frame.  The candidate is the entry with grid >= min_grid and the fewest links
 *   (then the larger grid, then the lower slot); start_px = the corners of G minus p4.  None: HNET_RV_NO_CANDIDATE, rec zero, start_px quiet NaNs.
 *   The alignment candidate -> curr runs from start_px; `rec` is its level-0 record, byte for byte hnet_op_photo_align_robust(stored keyframe, curr,
 *   start_px) with the same options.  REJECTED, one reason bit, in this order: HNET_RV_STOPPED (rec stopped SINGULAR, DEGENERATE or FEW_PIXELS);
 *   HNET_RV_MSE_ABOVE_MAX (max_mse > 0 and not mse <= max_mse); HNET_RV_NON_FINITE (an offset of rec); HNET_RV_LOW_OVERLAP (n_valid / 71 680 <
 *   min_overlap); HNET_RV_CLOSURE_ABOVE_MAX (max_closure_px > 0 and the worst |offset - start| exceeds it: a false match inside the basin);
 *   HNET_RV_CHAIN (H(offsets) . entry.h_origin_key is degenerate).  Else HNET_RV_ATTACHED: the stored keyframe becomes the session's keyframe again,
 *   key_px = rec's offsets, h_origin_key = the entry's, age = 0, keyframes unchanged; the next track measures against it, and the next re-key has the
 *   entry's links + 1.  A rejected or candidate-less revisit changes nothing.
 * Read-only for everything else, like a track.  Errors, nothing changed and nothing written: everything hnet_sessions_keyframe_track refuses (with
 * min_grid outside 1 .. 64, min_overlap outside 0 .. 1, a negative or non-finite max_mse or max_closure_px for its own options); HNET_ERR_INVALID_ARG
 * before hnet_sessions_enable_keyframe_map; HNET_ERR_NOT_READY for a listed session without a keyframe or with an image its last track did not see.
 * hnet_sessions_enable_keyframe_map: once, after hnet_sessions_enable_keyframes and before any session holds a keyframe (HNET_ERR_INVALID_ARG
 * otherwise, and for a capacity outside 2 .. 8); allocates [n_sessions][capacity][71 680] bytes (zeroed), the entries, the map states and per-slot
 * scratch for max_batch.  A revisit is ONE upload {ids | curr slot}, 4 small launches around the alignment's sequence (select, gather, decide, attach),
 * ONE download of the records [n] and one synchronisation; a track with a map has 2 small launches more (note, store). */
typedef struct hnet_keyframe_revisit_opts {
    hnet_photo_robust_opts align;
    int32_t levels;            /* 1 .. 4 */
    int32_t min_grid;          /* 1 .. 64 */
    double  min_overlap;       /* 0 .. 1 */
    double  max_mse;           /* >= 0; 0 = no limit */
    double  max_closure_px;    /* >= 0; 0 = no limit */
} hnet_keyframe_revisit_opts;
enum { HNET_RV_NO_CANDIDATE = 1, HNET_RV_ATTACHED = 2,
       HNET_RV_STOPPED = 4, HNET_RV_MSE_ABOVE_MAX = 8, HNET_RV_NON_FINITE = 16, HNET_RV_LOW_OVERLAP = 32, HNET_RV_CLOSURE_ABOVE_MAX = 64,
       HNET_RV_CHAIN = 128,                                                                              /* the REJECTED reasons, in the order tested */
       HNET_RV_REJECTED = 4 | 8 | 16 | 32 | 64 | 128 };
typedef struct hnet_keyframe_map_entry { int32_t valid, links, serial, pad; double h_origin_key[9]; } hnet_keyframe_map_entry;
typedef struct hnet_keyframe_map_state { int32_t cur_slot /* the held keyframe's slot, -1: not in the map */, cur_links, cursor, serial; } hnet_keyframe_map_state;
typedef struct hnet_keyframe_revisit {
    hnet_photo_robust rec;       /* level 0, stored keyframe -> curr; zeros without a candidate */
    float   start_px[8];         /* what the alignment started from (quiet NaNs: no candidate) */
    float   key_px[8];           /* the session's key_px after the call: rec's offsets when attached, else unchanged */
    double  h_origin_before[9];  /* origin -> curr by the chain as it was */
    double  h_origin_curr[9];    /* origin -> curr after the call: through the candidate when attached, else h_origin_before */
    double  closure_px[8];       /* corners of h_origin_curr minus corners of h_origin_before: the drift the attach removed; zeros unless attached */
    double  overlap;             /* rec.px.n_valid / 71 680; 0 without a candidate */
    int32_t slot, links, grid;   /* the candidate's; -1, 0, 0 without one */
    int32_t flags;               /* HNET_RV_* */
    int32_t pad[2];              /* written zero: records compare byte for byte */
} hnet_keyframe_revisit;
void hnet_keyframe_revisit_default_opts(hnet_keyframe_revisit_opts* o);  /* robust defaults, levels 3, min_grid 32, min_overlap 0.5, max_mse 0, max_closure_px 0 */
int  hnet_sessions_enable_keyframe_map(hnet_sessions* s, int capacity);
int  hnet_sessions_keyframe_revisit(hnet_sessions* s, int n, const int32_t* ids, const hnet_keyframe_revisit_opts* opts, hnet_keyframe_revisit* out /* [n] */);
/* operator level (tests): the session's entries [capacity] and map state; a stored image, 224 x 320 bytes, whatever the entry's validity (zeros when the
 * slot was never written).  One download, one synchronisation each.  HNET_ERR_INVALID_ARG before hnet_sessions_enable_keyframe_map. */
int  hnet_sessions_keyframe_map_info(hnet_sessions* s, int id, hnet_keyframe_map_entry* entries /* [capacity] */, hnet_keyframe_map_state* map_state);
int  hnet_sessions_get_map_keyframe(hnet_sessions* s, int id, int slot, uint8_t* out);

/* ---- a start that needs no prediction: a coarse search over integer translations, and finding a lost camera among its keyframes, on the device
 * (csrc/kernels_photo_search.hip; the shared code is include/hnet_photo_search.h and include/hnet_keyframe_reloc.h).  Opt-in: a program that
 * never calls these entry points allocates, launches and returns exactly what it did before.
 * Every alignment above needs a start inside its basin (about 24 px at four levels), and both the track and the revisit get theirs from a prediction.
 * The search compares the level-3 thumbnails (40 x 28 u8, level 3 of the pyramid of hnet_op_photo_pyramid bit for bit) of img1 and img2 at every integer
 * shift (dx, dy), |dx| <= radius_x <= 30, |dy| <= radius_y <= 20, 8 full-resolution pixels per step: template pixel (u, v) of img1 against img2 at
 * (u + dx, v + dy), the sense of H(x).  Over the overlap (n pixels) the integer sums Sa, Sb, Sab, Saa, Sbb give, exact in int64, num = n Sab - Sa Sb,
 * va = n Saa - Sa^2, vb = n Sbb - Sb^2; a shift is SCORED when n >= min_overlap, va > 0 and vb > 0, score = (double) num / sqrt((double) va * (double) vb).
 * The best: highest score, then smaller dx^2 + dy^2, then smaller dy, then smaller dx.  `second` is the best by the same order among the scored shifts
 * more than one step from it in x or y; -1 when there is none.  Flags, exactly one, in this order: HNET_PS_NO_TEXTURE (nothing was scored: a constant
 * thumbnail, or a min_overlap nothing meets; dx = dy = 0, score -1, sums 0), HNET_PS_LOW_SCORE (score < min_score), HNET_PS_AMBIGUOUS
 * (score - second < min_margin), else HNET_PS_FOUND.  start_px is (8 dx, 8 dy) on all four corners when FOUND, quiet NaNs otherwise (on which the
 * alignments report HNET_ALIGN_DEGENERATE at once).  The defaults were set between the figures of a prototype on synthetic views, not calibrated on
 * footage.  A record depends on its pair and the options alone.
 * Errors, nothing written: HNET_ERR_INVALID_ARG for a null argument, n < 1 or options out of range (radius_x outside 0 .. 30, radius_y outside 0 .. 20,
 * min_overlap outside 16 .. 1120, min_score outside -1 .. 1, min_margin outside 0 .. 2, a NaN); HNET_ERR_CAPACITY for n > max_batch.  One upload, two
 * launches (thumbnails, search), one download, one synchronisation. */
typedef struct hnet_photo_search_opts {
    int32_t radius_x;          /* 0 .. 30 level-3 pixels */
    int32_t radius_y;          /* 0 .. 20 */
    int32_t min_overlap;       /* 16 .. 1120 level-3 pixels */
    int32_t pad;
    double  min_score;         /* -1 .. 1 */
    double  min_margin;        /* 0 .. 2 */
} hnet_photo_search_opts;
enum { HNET_PS_FOUND = 1, HNET_PS_NO_TEXTURE = 2, HNET_PS_LOW_SCORE = 4, HNET_PS_AMBIGUOUS = 8 };
#define HNET_PS_SHIFTS_X 61
#define HNET_PS_SHIFTS_Y 41
typedef struct hnet_photo_search {
    float   start_px[8];       /* (8 dx, 8 dy) on the four corners when FOUND, else quiet NaNs */
    int32_t dx, dy;            /* the best shift, level-3 pixels */
    int32_t dx2, dy2;          /* the second's shift; 0, 0 without one */
    int32_t n_overlap;         /* pixels of the best shift's overlap */
    int32_t flags;             /* HNET_PS_* */
    double  score, second;     /* -1 without one */
    int32_t sa, sb, sab, saa, sbb;     /* the sums of the best shift */
    int32_t pad;               /* written zero: records compare byte for byte */
} hnet_photo_search;
void hnet_photo_search_default_opts(hnet_photo_search_opts* o);      /* 30, 20, 140, 0.75, 0.1 */
/* operator call, host pointers: img1 / img2 u8 [n][224][320], out [n]; scores_out NULL or double [n][41][61], index [dy + 20][dx + 30]: the score of every
 * shift of the full range, quiet NaN where a shift is not scored or lies outside the radii (operator level, for the tests) */
int  hnet_op_photo_search(hnet_ctx* ctx, const uint8_t* img1, const uint8_t* img2, int n, const hnet_photo_search_opts* opts, hnet_photo_search* out,
                          double* scores_out);
/* the same on the (prev, curr) pair of each listed session, byte for byte the operator call; read-only like hnet_sessions_photo_align_robust, errors as
 * there */
int  hnet_sessions_photo_search(hnet_sessions* s, int n, const int32_t* ids, const hnet_photo_search_opts* opts, hnet_photo_search* out);

/* hnet_sessions_keyframe_relocalise: after hnet_sessions_enable_keyframes, with or without a map.  The intended use: track, see HNET_KF_LOST, relocalise
 * on the same frame.  The candidates of a listed session are its held keyframe (target -1) and, with a map, every valid entry with slot != cur_slot
 * (target = the slot); there is no condition on links and no chain prediction.  Every candidate is searched against the session's current frame
 * (candidate = img1).  The pick is the FOUND candidate of the highest score; ties go to the held keyframe, then the lower slot.  None:
 * HNET_RL_NO_CANDIDATE, target -2, nothing changes.  Otherwise the alignment candidate -> curr runs from the search's start_px with
 * hnet_op_photo_align_robust's launch sequence, rv.rec being its level-0 record byte for byte, and one decision follows on the device.
 *   A map entry: the decision of hnet_sessions_keyframe_revisit exactly as it is, with the searched start in place of the selected one; the reasons and
 *   effects are unchanged, HNET_RL_ATTACHED re-anchors h_origin_key to the entry's.  rv.grid is 0.
 *   The held keyframe: the same REJECTED reasons in the same order without HNET_RL_CHAIN; else HNET_RL_RETRACKED: key_px = rec's offsets, everything
 *   else of the state and the map state unchanged.  rv.slot = -1, rv.links = 0; rv.h_origin_curr = H(key_px) . h_origin_key (h_origin_before when that
 *   product is degenerate or the call is rejected), rv.closure_px as hnet_keyframe_revisit defines it.
 * A rejected or candidate-less call changes neither state.  Read-only for everything else, like a track.
 * Errors, nothing changed and nothing written: everything hnet_sessions_keyframe_revisit refuses except that the map need not be enabled (min_grid does
 * not exist here); the search options out of range; HNET_ERR_NOT_READY for a listed session without a keyframe or whose latest image is not the one its
 * last track saw.  The first call allocates the thumbnails and records of max_batch x 9 candidates.  A call is ONE upload {ids | curr slot}, the
 * launches (thumbnails, search, pick, gather, the alignment's sequence, decide, and the map's attach), ONE download of the records [n] and one
 * synchronisation; hnet_sessions_last_keyframe_device_ms covers it. */
typedef struct hnet_keyframe_relocalise_opts {
    hnet_photo_robust_opts align;
    int32_t levels;            /* 1 .. 4 */
    int32_t pad;
    hnet_photo_search_opts search;
    double  min_overlap;       /* 0 .. 1 */
    double  max_mse;           /* >= 0; 0 = no limit */
    double  max_closure_px;    /* >= 0; 0 = no limit: the worst |offset - searched start| */
} hnet_keyframe_relocalise_opts;
enum { HNET_RL_NO_CANDIDATE = 1, HNET_RL_ATTACHED = 2,
       HNET_RL_STOPPED = 4, HNET_RL_MSE_ABOVE_MAX = 8, HNET_RL_NON_FINITE = 16, HNET_RL_LOW_OVERLAP = 32, HNET_RL_CLOSURE_ABOVE_MAX = 64,
       HNET_RL_CHAIN = 128,                                                                              /* the REJECTED reasons: HNET_RV_*'s values */
       HNET_RL_RETRACKED = 256,
       HNET_RL_REJECTED = 4 | 8 | 16 | 32 | 64 | 128 };
typedef struct hnet_keyframe_relocalise {
    hnet_keyframe_revisit rv;    /* the alignment's level-0 record, start_px, key_px, h_origin_before / _curr, closure_px, overlap, slot, links; flags HNET_RL_* */
    hnet_photo_search search;    /* of the picked candidate; all zero without a pick */
    int32_t target;              /* -1: the held keyframe, >= 0: the map slot, -2: no pick */
    int32_t n_searched;          /* candidates searched */
    int32_t n_found;             /* of them HNET_PS_FOUND */
    int32_t pad;                 /* written zero */
} hnet_keyframe_relocalise;
void hnet_keyframe_relocalise_default_opts(hnet_keyframe_relocalise_opts* o);  /* robust defaults, levels 4, search defaults, min_overlap 0.5, max_mse 0, max_closure_px 0 */
int  hnet_sessions_keyframe_relocalise(hnet_sessions* s, int n, const int32_t* ids, const hnet_keyframe_relocalise_opts* opts,
                                       hnet_keyframe_relocalise* out /* [n] */);

/* ---- the same search under a table of ORIENTATION hypotheses: a camera that is lost and has turned (csrc/kernels_photo_search_oriented.hip; the shared
 * code is include/hnet_photo_search_oriented.h).  Opt-in like the search above.
 * A hypothesis is a linear map A about the frame centre c = (159.5, 111.5), x' = c + A (x - c) + t in the sense of H(x): a table entry holds A (a, row
 * major) and b = round(65536 A^-1).  hnet_photo_search_make_hyp fills one from an angle and a scale in [0.5, 2] on the host; the device never evaluates a
 * trigonometric function.  A table has 1 .. 64 entries; hnet_photo_search_yaw_table fills `count` entries of scale 1 at first_deg + k step_deg degrees; the
 * documented default is 60 entries of 6 degrees from -180.
 * Per entry the template thumbnail is warped by b in integers (bilinear in 1/256 steps; a pixel whose taps leave the thumbnail is masked out), and the
 * search above runs with the sums restricted to the valid template pixels: n = sum m, Sa = sum a, Saa = sum a^2, Sab = sum a b, Sb = sum m b,
 * Sbb = sum m b^2, the same score, best and second.  The winner over the table is the entry with the highest best score, ties to the lower index; the
 * flags are the four above, judged on the winner's best and its OWN second; nothing scored under any entry: HNET_PS_NO_TEXTURE.  The runner-up (hyp2,
 * score2: the best of the other entries) is reported and never gated: neighbouring entries are near-peaks by construction.  start_px at corner x_i is
 * c + A (x_i - c) + 8 (dx, dy) - x_i when FOUND, quiet NaNs otherwise.  With a table of only the identity, `base` is hnet_op_photo_search's record byte
 * for byte.
 * Errors, nothing written and nothing enqueued: those of hnet_op_photo_search; HNET_ERR_INVALID_ARG for a null table, n_hyp outside 1 .. 64, an entry with
 * a non-finite a or |b[i]| > 2 * 65536.  One upload, three launches (thumbnails, search, winner), one download, one synchronisation. */
#define HNET_PS_MAX_HYP 64
typedef struct hnet_photo_search_hyp {
    double  a[4];              /* A, row major */
    int32_t b[4];              /* round(65536 A^-1), row major */
} hnet_photo_search_hyp;
typedef struct hnet_photo_search_oriented {
    hnet_photo_search base;    /* of the winning entry; start_px under the entry */
    int32_t hyp;               /* the winner's table index; -1 without one */
    int32_t n_scored;          /* entries with a scored shift */
    int32_t hyp2;              /* the runner-up's table index; -1 without one */
    int32_t pad0;              /* written zero */
    double  score2;            /* the runner-up's best score; -1 without one */
    double  a[4];              /* the winner's A; zeros without one */
    int32_t pad[2];            /* written zero */
} hnet_photo_search_oriented;
/* 1 on success; 0, nothing written, for a non-finite angle or a scale outside [0.5, 2] */
int  hnet_photo_search_make_hyp(double angle_rad, double scale, hnet_photo_search_hyp* out);
/* 1 on success; 0 for a count outside 1 .. 64, a null table or a non-finite angle */
int  hnet_photo_search_yaw_table(double first_deg, double step_deg, int count, hnet_photo_search_hyp* out /* [count] */);
/* the documented default: 60 entries of 6 degrees from -180; returns the count (60), 0 for a null table */
#define HNET_PS_DEFAULT_HYP 60
int  hnet_photo_search_default_yaw_table(hnet_photo_search_hyp* out /* [60] */);
/* operator call, host pointers: as hnet_op_photo_search; hyps [n_hyp]; scores_out NULL or double [n][n_hyp][41][61] */
int  hnet_op_photo_search_oriented(hnet_ctx* ctx, const uint8_t* img1, const uint8_t* img2, int n, const hnet_photo_search_opts* opts,
                                   const hnet_photo_search_hyp* hyps, int n_hyp, hnet_photo_search_oriented* out, double* scores_out);
/* the same on the (prev, curr) pair of each listed session, byte for byte the operator call; read-only, errors as hnet_sessions_photo_search */
int  hnet_sessions_photo_search_oriented(hnet_sessions* s, int n, const int32_t* ids, const hnet_photo_search_opts* opts, const hnet_photo_search_hyp* hyps,
                                         int n_hyp, hnet_photo_search_oriented* out);

/* hnet_sessions_keyframe_relocalise_oriented: hnet_sessions_keyframe_relocalise with the oriented search over the same candidates; the pick, the
 * alignment from the searched start, the decision and the attach are that call's, unchanged, and so are its options and its refusals, plus the table's.
 * The first call allocates its scratch (the entries' records of max_batch x 9 candidates x 64 entries) before anything is enqueued.  A call is ONE upload
 * {ids | curr slot | table}, the launches (thumbnails, search, winner, pick, gather, the alignment's sequence, decide, and the map's attach), ONE
 * download and one synchronisation; hnet_sessions_last_keyframe_device_ms covers it. */
typedef struct hnet_keyframe_relocalise_oriented {
    hnet_keyframe_revisit rv;             /* as hnet_keyframe_relocalise */
    hnet_photo_search_oriented search;    /* of the picked candidate; all zero without a pick */
    int32_t target, n_searched, n_found;  /* as hnet_keyframe_relocalise */
    int32_t pad;                          /* written zero */
} hnet_keyframe_relocalise_oriented;
int  hnet_sessions_keyframe_relocalise_oriented(hnet_sessions* s, int n, const int32_t* ids, const hnet_keyframe_relocalise_opts* opts,
                                                const hnet_photo_search_hyp* hyps, int n_hyp, hnet_keyframe_relocalise_oriented* out /* [n] */);

/* ---- a FINE stage around the oriented winner, on level-2 thumbnails (csrc/kernels_photo_search_fine.hip; the shared code is
 * include/hnet_photo_search_fine.h).  Opt-in like the searches above: a program that never calls these allocates, launches and returns what it did.
 * The oriented search hands the alignment a start that is wrong by up to half a table step plus 4 px of the level-3 shift.  The fine stage runs on the
 * 80 x 56 level-2 thumbnails (level 2 of the alignment's pyramid bit for bit): n_fine sub-step entries fine[hyp][0 .. n_fine) around the winning entry
 * `hyp`, each over the shifts (2 dx + ex, 2 dy + ey) with |ex|, |ey| <= radius around twice the winning shift, warped and summed as the oriented search
 * does (the constants 79 / 55 in place of 39 / 27) and scored by the same score under 4 * opts.min_overlap.  The best over (entry j, ex, ey): the highest
 * score, then the smaller ex^2 + ey^2, then the smaller ey, then the smaller ex, then the lower j.
 * The fine table is [n_hyp][n_fine] entries, 1 <= n_fine <= 9, row h for coarse entry h; only the winner's row is read.
 * hnet_photo_search_fine_yaw_table fills entry [h][j] at (first_deg + h step_deg) + (j - (n_fine - 1) / 2) (step_deg / n_fine) degrees, scale 1: the table
 * that matches hnet_photo_search_yaw_table(first_deg, step_deg, count); for odd n_fine its middle column is that table byte for byte.
 * Flags of the fine part, exactly one, in this order: HNET_PSF_SKIPPED (the coarse record is not HNET_PS_FOUND: j = -1, ex = ey = sx = sy = 0, score -1,
 * a and sums 0, start_px quiet NaNs), HNET_PSF_NOTHING_SCORED (the same values; start_px is the coarse start_px unchanged), HNET_PSF_LOW_SCORE (the best
 * fine score is below min_score: the rejected best is reported; start_px is the coarse start_px unchanged), else HNET_PSF_REFINED: start_px at corner x_i
 * is c + A_f (x_i - c) + 4 (sx, sy) - x_i.  Scores of the two levels are never compared.  min_score defaults to the coarse 0.75 and is not calibrated.
 * Errors, nothing written and nothing enqueued: those of hnet_op_photo_search_oriented; HNET_ERR_INVALID_ARG for null fine options or a null fine table,
 * n_fine outside 1 .. 9, radius outside 0 .. 4, min_score outside [-1, 1] or NaN, a fine entry with a non-finite a or |b[i]| > 2 * 65536.
 * One upload, six launches (both thumbnails, search, winner, fine search, fine winner), one download, one synchronisation. */
enum { HNET_PSF_REFINED = 1, HNET_PSF_SKIPPED = 2, HNET_PSF_NOTHING_SCORED = 4, HNET_PSF_LOW_SCORE = 8 };
#define HNET_PSF_MAX_FINE 9
#define HNET_PSF_MAX_RADIUS 4
typedef struct hnet_photo_search_fine_opts {
    int32_t radius;            /* 0 .. 4 level-2 pixels around twice the coarse shift */
    int32_t n_fine;            /* 1 .. 9 entries per row of the fine table */
    double  min_score;         /* the lowest fine score of HNET_PSF_REFINED */
    int32_t pad[2];            /* ignored */
} hnet_photo_search_fine_opts;
typedef struct hnet_photo_search_fine_part {
    float   start_px[8];       /* the FINAL start for the alignment */
    int32_t flags;             /* HNET_PSF_* */
    int32_t j, ex, ey;         /* the best fine entry and its offsets */
    int32_t sx, sy;            /* the level-2 shift (2 dx + ex, 2 dy + ey) */
    int32_t n_overlap;         /* valid template pixels of the overlap of the best */
    int32_t pad0;              /* written zero */
    double  score;             /* of the best; -1 without one */
    double  a[4];              /* the fine entry's A; zeros without one */
    int32_t sa, sb, sab, saa, sbb;     /* the sums of the best */
    int32_t pad1;              /* written zero */
} hnet_photo_search_fine_part;
typedef struct hnet_photo_search_fine {
    hnet_photo_search_oriented coarse;   /* byte for byte hnet_op_photo_search_oriented's record */
    hnet_photo_search_fine_part fine;
} hnet_photo_search_fine;
void hnet_photo_search_fine_default_opts(hnet_photo_search_fine_opts* o);      /* radius 3, n_fine 5, min_score 0.75 */
/* 1 on success; 0 for a count outside 1 .. 64, n_fine outside 1 .. 9, a null table or a non-finite angle */
int  hnet_photo_search_fine_yaw_table(double first_deg, double step_deg, int count, int n_fine, hnet_photo_search_hyp* out /* [count][n_fine] */);
/* operator call, host pointers: as hnet_op_photo_search_oriented; fine [n_hyp][fine_opts->n_fine]; scores_out NULL or double [n][n_fine][9][9], index
 * (ey + 4) * 9 + (ex + 4), quiet NaN where a shift is not scored or lies outside the radius */
int  hnet_op_photo_search_fine(hnet_ctx* ctx, const uint8_t* img1, const uint8_t* img2, int n, const hnet_photo_search_opts* opts,
                               const hnet_photo_search_hyp* hyps, int n_hyp, const hnet_photo_search_fine_opts* fine_opts, const hnet_photo_search_hyp* fine,
                               hnet_photo_search_fine* out, double* scores_out);
/* the same on the (prev, curr) pair of each listed session, byte for byte the operator call; read-only, errors as hnet_sessions_photo_search_oriented */
int  hnet_sessions_photo_search_fine(hnet_sessions* s, int n, const int32_t* ids, const hnet_photo_search_opts* opts, const hnet_photo_search_hyp* hyps,
                                     int n_hyp, const hnet_photo_search_fine_opts* fine_opts, const hnet_photo_search_hyp* fine, hnet_photo_search_fine* out);

/* hnet_sessions_keyframe_relocalise_fine: hnet_sessions_keyframe_relocalise_oriented with the fine stage on the PICKED candidate only: after the pick and
 * the gather, the level-2 thumbnails of the candidate and the current frame, the fine search and its winner, which writes the final start over the
 * alignment's start.  The alignment, the decision and the attach are that call's, unchanged; `base` is its record (rv.start_px is the final start) and
 * `fine` the fine part, HNET_PSF_SKIPPED with a quiet-NaN start for a slot without a pick.  With a coarser table (30 entries of 12 degrees) the call costs
 * less than the oriented one under its default table and starts the alignment closer.  Refusals: that call's and the fine ones above.  The
 * first call allocates the fine scratch of its own before anything is enqueued.  ONE upload {ids | curr slot | table | fine table}, ONE download and one
 * synchronisation; hnet_sessions_last_keyframe_device_ms covers it. */
typedef struct hnet_keyframe_relocalise_fine {
    hnet_keyframe_relocalise_oriented base;
    hnet_photo_search_fine_part fine;
} hnet_keyframe_relocalise_fine;
int  hnet_sessions_keyframe_relocalise_fine(hnet_sessions* s, int n, const int32_t* ids, const hnet_keyframe_relocalise_opts* opts,
                                            const hnet_photo_search_hyp* hyps, int n_hyp, const hnet_photo_search_fine_opts* fine_opts,
                                            const hnet_photo_search_hyp* fine, hnet_keyframe_relocalise_fine* out /* [n] */);

/* ---- sessions, recovering a lost camera INSIDE the track, before the bridge (csrc/kernels_keyframe_recover.hip; the shared code is
 * include/hnet_keyframe_recover.h).  Opt-in: a program that never calls hnet_sessions_keyframe_track_recover allocates, launches and returns
 * what it did before.  hnet_sessions_keyframe_track with auto_rekey commits its verdict in the same call: a LOST frame becomes the keyframe and the origin
 * chain takes a link of dead reckoning, after which a relocalise finds the current frame on itself.  This call is that track with the oriented
 * relocalisation run between the LOST verdict and its commit.  Callable after hnet_sessions_enable_keyframes, with or without a map; hyps == NULL with
 * n_hyp == 0 is the identity entry alone.  Per listed session, independent of the other slots, with T1 = the track's decision under opts.track and T0 =
 * the same under opts.track with auto_rekey = 0, both on the state before the call:
 *   not LOST (HNET_KF_FIRST included): the state, `track`, the keyframe store and the map are exactly hnet_sessions_keyframe_track(opts.track)'s; `reloc`
 *     is all zero except target = -2.
 *   LOST: the session takes T0's state (the keyframe stays, key_px is the bridge, the age grows by one) and the map's note runs on T0's flags (a restart
 *     invalidates the entries before they are searched); then hnet_sessions_keyframe_relocalise_oriented(opts.reloc, hyps) runs on that state against the
 *     current frame exactly as it is, and `reloc` is its record byte for byte.
 *     HNET_RL_RETRACKED or HNET_RL_ATTACHED: the state is what that call leaves (key_px = reloc.rv.key_px); `track` is T0's record with HNET_KF_RECOVERED
 *       or-ed into flags: rec, start_px and the bridge in key_px are kept and show why the frame was lost.  No re-key is judged on a recovered frame: the
 *       next track judges overlap and age.
 *     HNET_RL_NO_CANDIDATE or a REJECTED reason: the state, `track`, the keyframe store and the map are exactly hnet_sessions_keyframe_track(opts.track)'s,
 *       i.e. T1 formed from the state before the call, for either value of auto_rekey.
 * The host bookkeeping moves as a track moves it: a relocalise or a revisit may follow at once.  Read-only for everything else, like a track.  Errors,
 * nothing changed, written or enqueued: everything hnet_sessions_keyframe_track refuses, and the option and table refusals of
 * hnet_sessions_keyframe_relocalise_oriented.  The first call allocates its scratch before anything is enqueued.  A call is ONE upload
 * {step | ids | curr slot | gap | table}, the track's launches with the decision deferred, the relocalisation's launches with the candidates of the
 * sessions that are not lost marked absent (those ride through on quiet-NaN starts), a finish, a second commit for the unrecovered sessions, ONE download
 * and one synchronisation; hnet_sessions_last_keyframe_device_ms covers it. */
enum { HNET_KF_RECOVERED = 2048 };
typedef struct hnet_keyframe_recover_opts { hnet_keyframe_opts track; hnet_keyframe_relocalise_opts reloc; } hnet_keyframe_recover_opts;
typedef struct hnet_keyframe_recover { hnet_keyframe_track track; hnet_keyframe_relocalise_oriented reloc; } hnet_keyframe_recover;
void hnet_keyframe_recover_default_opts(hnet_keyframe_recover_opts* o);   /* the two defaults, and track.max_mse stays 0: the caller chooses it */
int  hnet_sessions_keyframe_track_recover(hnet_sessions* s, int n, const int32_t* ids, const float* step_px /* [n][8] or NULL, as the track's */,
                                          const hnet_keyframe_recover_opts* opts, const hnet_photo_search_hyp* hyps, int n_hyp,
                                          hnet_keyframe_recover* out /* [n] */);

/* ---- hnet_filters: a session's keyframe track as a filter measurement, INSIDE the step (csrc/kernels_filters_keyframe.hip; the shared code is
 * include/hnet_keyframe_measure.h).  Per session and off by default.  The keyframe layers above measure every camera without drift, but the
 * filter resets its offset states (and their covariance) after every update: a keyframe result handed over after hnet_filters_step meets H P H^T = 0
 * and carries nothing.  With the feature on, a stepping session's step instead ends like this, hnet_ekf::iterated_update_keyframe_measured:
 *   step_px = (float)(159.5 * offset) of the state after the network's iterations (the last one's update then runs with update_offset = 1: rows 0 .. 14
 *     of dx do not depend on it and the offsets are reset afterwards, so every other session keeps its bytes);
 *   hnet_sessions_keyframe_track with that step: start_px = compose(step_px, key_px), the robust alignment key -> curr, the unchanged rule with
 *     opts.track and the session's gap.  The keyframe state, the store and, with a map enabled, its entries end exactly as that call leaves them;
 *   z_px = the corners of H(track.rec offsets) . inverse(H(key_px before the track)) minus p4, rounded to fp32: the CONSECUTIVE-frame offsets the
 *     network measures and the offset states predict, but with errors that telescope - the composition of the H(z_px) over a stay on one keyframe is
 *     the last key_px, whatever the individual errors were;
 *   R_px = cov_scale * mse * inverse(info8) + sigma_floor_px^2 I, symmetrised, as hnet_filters_set_photo_refine forms it; cov_scale is the CALLER's and
 *     has no default.  Two approximations are deliberate: the Jacobian of z_px with respect to the new key_px is taken as I, and the noise of the
 *     previous key_px is ignored (which is what lets the errors telescope);
 *   the packed record {z_px | (float)(R_px / k_net_cov)} goes to the unchanged innovation (with the session's NIS gate, when set) and update kernels,
 *     against the prior of the current state, with update_offset = 0; the reset follows.
 * The measurement is UNUSABLE and nothing is applied when (one reason bit each, tested in this order) the session held no keyframe before the call
 * (HNET_KFM_FIRST); the track's record has a LOST bit; it has HNET_KF_GAP; the session's previous in-step track left no measured key_px
 * (HNET_KFM_PREV_NOT_MEASURED: a word per session, 1 after TRACKED or FIRST, 0 after LOST and for a session never measured; a reset of the keyframe
 * makes the next track FIRST); H(key_px before) has no inverse (|det| below 1e-12 of the cube of its largest entry in frame units:
 * include/hnet_keyframe_map.h inverse) or a corner of the product has z <= 0 or is not finite; then hnet_filters_set_photo_refine's reasons on the level-0 record, in their order.
 * `when`: HNET_KFM_ALWAYS applies a usable measurement after whatever the network's iterations did; HNET_KFM_IF_NONE only when they applied nothing
 * (the slot's update counter is 0).  After a singular S of the network's own neither applies.  A usable measurement kept out is HNET_KFM_NOT_SELECTED.
 * updates[i] counts the keyframe update; its S found singular is the existing -1 - applied.  Every other record keeps its shape and content.
 * A step or advance in which at least one STEPPING session measures enqueues, for all its stepping sessions, 3 small kernels, the track's launches (the
 * keyframe gathered into a buffer of the feature's own: the context's staging keeps the consecutive pair), one prior, one innovation and one update
 * launch, inside the attempt and inside hnet_filters_last_timing's device window; the track's commits (state table, new keyframe images, map note and
 * store) and the prev_ok words follow the ACCEPTED attempt, stream ordered, without a second synchronisation: a repeated attempt leaves what a single
 * one leaves.  Still one upload, one download, one synchronisation.  Any other call launches exactly what it launched before.
 * HNET_ERR_INVALID_ARG from the step or advance, nothing changed: stepping sessions that measure with different opts.track (one launch sequence serves
 * them all; the measurement's own fields are per session), or measuring and refining (hnet_filters_set_photo_refine) sessions in one call. */
enum { HNET_KFM_ALWAYS = 0, HNET_KFM_IF_NONE = 1 };
typedef struct hnet_keyframe_measure_opts {
    hnet_keyframe_opts track;  /* the in-step track's options */
    double  cov_scale;         /* > 0; hnet_keyframe_measure_default_opts leaves 0 on purpose: the caller must choose it */
    double  sigma_floor_px;    /* >= 0: sigma_floor_px^2 is added to the diagonal of R_px */
    double  max_mse;           /* 0 = no limit; else a record with px.mse above it is unusable (the track's own limit is track.max_mse) */
    int32_t when;              /* HNET_KFM_ALWAYS / HNET_KFM_IF_NONE */
    int32_t pad;
} hnet_keyframe_measure_opts;
void hnet_keyframe_measure_default_opts(hnet_keyframe_measure_opts* o);      /* keyframe defaults, 0 (!), 0.05, 0, ALWAYS */
enum { HNET_KFM_ASKED = 1,               /* the session measures: `track` is its in-step track's record */
       HNET_KFM_APPLIED = 2,             /* the keyframe update was applied */
       HNET_KFM_NIS_REJECTED = 4,        /* the session's NIS gate refused the measurement */
       HNET_KFM_S_SINGULAR = 8,          /* the measurement's S was singular */
       HNET_KFM_BAD_K_NET_COV = 16, HNET_KFM_STOPPED = 32, HNET_KFM_NO_STEP = 64, HNET_KFM_MSE_ABOVE_MAX = 128, HNET_KFM_NO_FACTOR = 256,
       HNET_KFM_NON_FINITE = 512,        /* HNET_REFINE_*'s reasons, tested last */
       HNET_KFM_FIRST = 1024, HNET_KFM_TRACK_LOST = 2048, HNET_KFM_TRACK_GAP = 4096, HNET_KFM_PREV_NOT_MEASURED = 8192, HNET_KFM_NO_INVERSE = 16384,
       HNET_KFM_NOT_SELECTED = 32768,    /* `when`, or a singular S of the network's own, kept the measurement out: not an UNUSABLE reason */
       HNET_KFM_UNUSABLE = 16 | 32 | 64 | 128 | 256 | 512 | 1024 | 2048 | 4096 | 8192 | 16384 };
typedef struct hnet_keyframe_measure {
    hnet_keyframe_track track; /* byte for byte hnet_sessions_keyframe_track's record for step_px */
    float   step_px[8];        /* the filter's own step */
    float   z_px[8];           /* zeros when unusable */
    double  r_px[64];          /* zeros when unusable */
    hnet_innovation innov;     /* of the keyframe measurement; iteration = max_iekf_iteration; HNET_INNOV_NONE (zeros) when unusable or not selected */
    int32_t flags;             /* HNET_KFM_*; 0 (and the whole record zero) for a session that does not measure */
    int32_t pad;               /* written as zero: records compare byte for byte */
} hnet_keyframe_measure;
/* opts == NULL turns the feature off for the session.  The first call with options allocates the feature's buffers and grows the output block
 * (hnet_filters_last_* have nothing to describe until the next step).  HNET_ERR_INVALID_ARG, nothing changed: a bad id, a call before
 * hnet_sessions_enable_keyframes, track options hnet_sessions_keyframe_track would refuse, cov_scale <= 0 or not finite, a negative or non-finite
 * sigma_floor_px or max_mse, a `when` that is neither value, a session with hnet_filters_set_photo_refine on (and that call refuses a measuring session). */
int  hnet_filters_set_keyframe_measure(hnet_filters* f, int id, const hnet_keyframe_measure_opts* opts);
/* the records [n] of the last step (n: its n) or advance (n: its STEPPED sessions, in the order listed).  A wrong n, or a last call that ran without a
 * measuring session: HNET_ERR_INVALID_ARG, nothing written */
int  hnet_filters_last_keyframe_measure(const hnet_filters* f, int n, hnet_keyframe_measure* out);
/* per session, accumulated on the host from the records of accepted calls only: asked, applied, unusable (any reason bit), nis_rejected; sum_nis /
 * max_nis over the measurements whose NIS was formed and finite: what a caller calibrates cov_scale with (a consistent filter gives a mean of 8). */
typedef struct hnet_keyframe_measure_stats { int64_t asked, applied, unusable, nis_rejected; double sum_nis, max_nis; } hnet_keyframe_measure_stats;
int  hnet_filters_keyframe_measure_stats(const hnet_filters* f, int id, hnet_keyframe_measure_stats* out);
int  hnet_filters_reset_keyframe_measure_stats(hnet_filters* f, int id);

/* ---- hnet_filters: recovering a lost camera INSIDE the in-step keyframe track (csrc/kernels_filters_keyframe_recover.hip; the shared code is
 * include/hnet_keyframe_measure_recover.h).  Per measuring session and off by default.  With auto_rekey = 1 a frame the in-step track judges
 * LOST is committed inside the step: the lost frame becomes the keyframe, the origin chain takes a link of dead reckoning and prev_ok goes to 0 - and
 * nothing can be put between the verdict and its commit from outside.  With the feature on, the session's in-step track becomes
 * hnet_sessions_keyframe_track_recover with the filter's own step_px, the session's gap, the measure options' `track` block and the reloc options and
 * table given here: a LOST session is relocalised (oriented) on T0's state before its re-key is committed.  The keyframe state, the store and the map
 * end byte for byte as that sessions call leaves them.  Then, in this order: HNET_KFM_FIRST; HNET_KFM_TRACK_LOST only for a LOST record without
 * HNET_KF_RECOVERED; HNET_KFM_REATTACHED when the relocalise re-attached the session to a map keyframe (HNET_RL_ATTACHED): the keyframe changed under
 * the session, the frame has no consecutive-frame meaning and is FIRST-like, nothing is applied; the remaining reasons as before.  A frame recovered on
 * its own keyframe (HNET_RL_RETRACKED) still measures: z_px and R_px are formed from the relocalise's level-0 record reloc.rv.rec (the trials accepted
 * over the levels of ITS alignment) against key_px before the call, and the informational HNET_KFM_FROM_RELOC is set.  Such a z_px may lie far from the
 * prior - a kidnapped camera really did move - and whether it is applied is the session's NIS gate's business.  prev_ok stays 1 after either recovery.
 * No fine stage runs inside the step and no re-key is judged on a recovered frame.  `when` applies unchanged.  The per-session statistics count
 * "unusable" with HNET_KFMR_UNUSABLE; without the feature the new bit never occurs.
 * A step or advance with at least one recovering STEPPING session enqueues hnet_sessions_keyframe_track_recover's launches in place of the track's, on
 * working copies of the state table and of the map's entries and states; every image write (the first commit, the attach, the second commit, both map
 * stores) follows the ACCEPTED attempt, stream ordered: a repeated attempt leaves what a single one leaves.  Still one upload, one download, one
 * synchronisation.  A call without a recovering stepping session launches exactly what it launched before.
 * HNET_ERR_INVALID_ARG from the step or advance, nothing changed: stepping recovering sessions whose reloc options or tables differ byte-wise. */
enum { HNET_KFM_FROM_RELOC = 65536,      /* the measurement was taken from the relocalise's record; informational */
       HNET_KFM_REATTACHED = 131072,     /* UNUSABLE: the frame was re-attached to a map keyframe */
       HNET_KFMR_UNUSABLE = HNET_KFM_UNUSABLE | 131072 };
typedef struct hnet_keyframe_measure_recover {
    hnet_keyframe_measure m;   /* m.track: byte for byte hnet_sessions_keyframe_track_recover's `track` for m.step_px */
    hnet_keyframe_relocalise_oriented reloc;   /* its `reloc`: all zero with target -2 for a session that needed no recovery or has the feature off */
} hnet_keyframe_measure_recover;
/* reloc == NULL turns recovery off for the session; hyps == NULL with n_hyp == 0 is the identity entry alone.  The table is copied.  The first call with
 * options allocates the feature's buffers and grows the output block (hnet_filters_last_* have nothing to describe until the next step).  Turning the
 * measurement off (hnet_filters_set_keyframe_measure with NULL) turns recovery off.  HNET_ERR_INVALID_ARG, nothing changed: a bad id, a session without
 * hnet_filters_set_keyframe_measure on, options or a table hnet_sessions_keyframe_relocalise_oriented would refuse.  A keyframe map may be enabled
 * before or after (while no session holds a keyframe, as always): the working copies of its tables come with whichever call is second. */
int  hnet_filters_set_keyframe_recover(hnet_filters* f, int id, const hnet_keyframe_relocalise_opts* reloc, const hnet_photo_search_hyp* hyps, int n_hyp);
/* hnet_filters_last_keyframe_measure's records with the relocalise records.  A wrong n, or a last call that ran without a recovering session:
 * HNET_ERR_INVALID_ARG, nothing written */
int  hnet_filters_last_keyframe_recover(const hnet_filters* f, int n, hnet_keyframe_measure_recover* out);

/* ---- a keyframe map RENDERED into a view, on the device (csrc/kernels_keyframe_render.hip; the shared code is include/hnet_keyframe_render.h;
 * DESIGN 7ab).  Every stored keyframe of a map carries h_origin_key; a view is a width x height u8 image with h_origin_view (origin -> view, h[8] = 1).
 * Each pixel of the view samples every stored keyframe it falls into (bilinear, the position in double), the samples are blended by `mode`, out_cover
 * holds how many keyframes covered the pixel, and the record counts, in integers, how far each keyframe's samples lie from what is displayed where two
 * or more overlap: sse[j] / n[j] is entry j's disagreement with the composite, and an entry whose h_origin_key is off stands out.  Read-only for every
 * state the sessions hold, and opt-in: a sessions object that never calls hnet_sessions_enable_keyframe_render allocates, launches and returns what it did. */
enum { HNET_RENDER_FEWEST_LINKS = 0,   /* the covering keyframe with the fewest chain links, then the lower slot: the least-drifted ground */
       HNET_RENDER_NEWEST = 1,         /* the covering keyframe with the largest serial */
       HNET_RENDER_MEAN = 2 };         /* (sum + cover / 2) / cover of the covering samples, in integers */
#define HNET_RENDER_MAX_DIM 8192       /* the largest width or height of a view */
typedef struct hnet_keyframe_render_opts { int32_t width, height, mode, pad; } hnet_keyframe_render_opts;
typedef struct hnet_keyframe_render_rec {
    double   h_origin_view[9];     /* the view that was rendered */
    uint64_t n_covered, n_overlap; /* pixels with cover >= 1, >= 2 */
    uint64_t n[8], sse[8];         /* per map slot, over the pixels with cover >= 2 it covers: their count and the sum of (sample - output)^2; zeros beyond capacity */
    int32_t  used_mask, skipped_mask;   /* the slots that took part; the slots below the capacity that did not (invalid, or no S: a singular matrix) */
} hnet_keyframe_render_rec;        /* every byte written: records compare byte for byte */
/* The view that shows all of a map: the corners of every valid entry taken to the origin frame, bounded, scaled uniformly and centred in the view with
 * margin_px free on every side.  Host side, in double.  0 (h_origin_view untouched): no usable entry, a box or a view without extent, a corner behind
 * the camera or a non-finite value; else 1. */
int  hnet_keyframe_render_fit_view(const hnet_keyframe_map_entry* entries, int capacity, int width, int height, double margin_px, double* h_origin_view /* [9] */);
/* Operator level: m (1 .. 8) caller-supplied images [m][224][320] and entries [m] rendered into ONE view; no session is involved.  out_img and
 * out_cover [height][width].  One upload, the two launches, one download, one synchronisation.  HNET_ERR_INVALID_ARG, nothing written: a null argument,
 * m outside 1 .. 8, a mode outside the three, width or height outside 1 .. HNET_RENDER_MAX_DIM, a non-finite entry of h_origin_view. */
int  hnet_op_keyframe_render(hnet_ctx* ctx, int m, const uint8_t* images, const hnet_keyframe_map_entry* entries, const double* h_origin_view /* [9] */,
                             const hnet_keyframe_render_opts* opts, uint8_t* out_img, uint8_t* out_cover, hnet_keyframe_render_rec* rec);
/* once, after hnet_sessions_enable_keyframe_map: the view and cover images of max_batch slots up to max_width x max_height, tables, pinned blocks and
 * events of its own.  HNET_ERR_INVALID_ARG: before the map, a second call, a maximum outside 1 .. HNET_RENDER_MAX_DIM. */
int  hnet_sessions_enable_keyframe_render(hnet_sessions* s, int max_width, int max_height);
/* The listed sessions' maps, each into its own view: h_origin_view [n][9], or NULL = each session's current frame as its origin chain predicts it
 * (h_origin_curr of its last track).  out_img and out_cover [n][height][width], out [n].  ONE upload, the two launches, ONE download and one
 * synchronisation; hnet_sessions_last_keyframe_device_ms covers it.  A session whose map has no valid entry is not an error: zeros, and a record that is
 * zero but for the view and skipped_mask.  Refused before anything is enqueued, nothing written: HNET_ERR_INVALID_ARG for a call before the enable, a null
 * argument, a mode outside the three, width or height below 1 or above the enabled maximum, a non-finite view entry, an id out of range or repeated;
 * HNET_ERR_CAPACITY for n > max_batch; HNET_ERR_NOT_READY for a NULL view on a session without a keyframe or whose latest image is not the one its last
 * track saw. */
int  hnet_sessions_keyframe_render(hnet_sessions* s, int n, const int32_t* ids, const double* h_origin_view, const hnet_keyframe_render_opts* opts,
                                   uint8_t* out_img, uint8_t* out_cover, hnet_keyframe_render_rec* out);

/* ---- a camera LOCALISED against its rendered keyframe map (csrc/kernels_keyframe_localise.hip; the shared code is include/hnet_keyframe_localise.h;
 * DESIGN 7ae).  A revisit measures against ONE stored keyframe and needs most of it in view; a camera between stored keyframes sees ground the map knows
 * and gets HNET_RV_NO_CANDIDATE.  The localise renders the entries into the view the chain predicts for the current frame (320 x 224, `mode`), takes the
 * cover image as the mask of hnet_op_photo_align_masked's alignment composite -> current frame from zero offsets, and judges the record: one flag, tested
 * in the order of the enum.  On HNET_LOC_LOCALISED h_origin_curr = H(offsets) . h_origin_before and correction_px = the corners of h_origin_curr minus those
 * of h_origin_before; otherwise h_origin_curr = h_origin_before and correction_px = 0.  When no entry took part or the cover is below min_cover nothing is
 * aligned (the start is quiet NaNs, the alignment returns at once) and `rec` is zero.  The defaults are choices, not measurements. */
enum { HNET_LOC_NO_MAP = 1,            /* no entry took part in the template */
       HNET_LOC_LOW_COVER = 2,         /* n_covered / 71 680 < min_cover */
       HNET_LOC_STOPPED = 4,           /* the record stopped SINGULAR, DEGENERATE or FEW_PIXELS */
       HNET_LOC_MSE_ABOVE_MAX = 8,     /* max_mse > 0 and not mse <= max_mse */
       HNET_LOC_NON_FINITE = 16,       /* an offset of the record is not finite */
       HNET_LOC_LOW_OVERLAP = 32,      /* n_valid / 71 680 < min_overlap */
       HNET_LOC_SHIFT_ABOVE_MAX = 64,  /* max_shift_px > 0 and the worst |offset| exceeds it */
       HNET_LOC_CHAIN = 128,           /* H(offsets) . h_origin_before is degenerate */
       HNET_LOC_LOCALISED = 256 };
typedef struct hnet_keyframe_localise_opts {
    hnet_photo_robust_opts align;
    int32_t levels, mode;              /* 1 .. 4 (3); HNET_RENDER_* (FEWEST_LINKS) */
    double  min_cover, min_overlap;    /* fractions of the frame (0.5, 0.4) */
    double  max_mse, max_shift_px;     /* 0 = no limit (0, 0) */
    int32_t apply, pad;                /* 0 / 1: hnet_sessions_keyframe_localise corrects the chain; the operator-level call has no state and ignores it */
} hnet_keyframe_localise_opts;
typedef struct hnet_keyframe_localise {
    hnet_photo_robust rec;             /* level 0 of the masked alignment, byte for byte hnet_op_photo_align_masked(template, cover, curr, 0) */
    double  h_origin_before[9], h_origin_curr[9], correction_px[8];
    double  cover, overlap;            /* n_covered and n_valid over 71 680 */
    int32_t used_mask, links_before, links, flags, pad[2];      /* links: 1 + the largest links in used_mask when localised */
} hnet_keyframe_localise;
void hnet_keyframe_localise_default_opts(hnet_keyframe_localise_opts* o);
/* Operator level: m (1 .. 8) caller-supplied images [m][224][320] and entries [m] (every valid entry is eligible), the predicted view h_origin_pred [9]
 * and the current frame curr [224][320]; no session is involved.  out_template / out_cover: NULL or [224][320], byte for byte hnet_op_keyframe_render's for
 * the same view, entries and mode.  ONE upload, the launch sequence {render setup, render, start, mask pyramid + masked alignment, decide}, ONE download,
 * one synchronisation.  HNET_ERR_INVALID_ARG, nothing written: a null argument but the last two, m outside 1 .. 8, options hnet_op_photo_align_robust
 * would refuse, levels outside 1 .. 4, a mode outside the three, min_cover or min_overlap outside 0 .. 1, a negative or non-finite max_mse or
 * max_shift_px, apply outside 0 / 1, a non-finite entry of h_origin_pred. */
int  hnet_op_keyframe_localise(hnet_ctx* ctx, int m, const uint8_t* images, const hnet_keyframe_map_entry* entries, const double* h_origin_pred /* [9] */,
                               const uint8_t* curr, const hnet_keyframe_localise_opts* opts, hnet_keyframe_localise* out, uint8_t* out_template,
                               uint8_t* out_cover);
/* once, after hnet_sessions_enable_keyframe_map (the render need not be enabled): templates, cover images, mask pyramids, tables and records of max_batch
 * slots, pinned blocks and events of its own.  A sessions object that never calls it allocates, launches and returns what it did.
 * HNET_ERR_INVALID_ARG: before the map, a second call. */
int  hnet_sessions_enable_keyframe_localise(hnet_sessions* s);
/* The listed sessions, each against its own map.  Eligible are the valid entries with slot != cur_slot and links < cur_links (the revisit's preference);
 * the view is the session's current frame as its origin chain predicts it (h_origin_curr of its last track) and the current frame its latest image.
 * links_before = cur_links.  With opts->apply = 1 a LOCALISED session's chain is corrected on the device: key_px stays,
 * h_origin_key <- inverse(H(key_px)) . h_origin_curr (HNET_LOC_CHAIN, nothing changed, if that product is degenerate), the map entry of cur_slot follows
 * when cur_slot >= 0, and cur_links and that entry's links become the record's links (1 + the largest links that took part: never more than before).  Age,
 * keyframe count, images, cursor and serial stay; the next track continues from the corrected chain.  A rejected call, apply = 0 and every unlisted session
 * change no byte of any state.  ONE upload {ids | current ring slots}, the launch sequence {render setup, eligible, render, gather + start, mask pyramid +
 * masked alignment, decide} on the context's staging and the store's alignment scratch, ONE download of out [n], one synchronisation;
 * hnet_sessions_last_keyframe_device_ms covers it.  Every id and ring slot is checked again on the device.  Refused before anything is enqueued, nothing
 * changed: everything hnet_sessions_keyframe_revisit refuses (with these options' rules for its own), and a call before the enable. */
int  hnet_sessions_keyframe_localise(hnet_sessions* s, int n, const int32_t* ids, const hnet_keyframe_localise_opts* opts, hnet_keyframe_localise* out /* [n] */);

/* ---- a keyframe map ADJUSTED jointly, on the device (csrc/kernels_keyframe_adjust.hip; the shared code is include/hnet_keyframe_adjust.h).
 * A revisit re-attaches the session to one stored keyframe; every entry stored in between keeps its drifted h_origin_key.  The adjustment re-measures
 * every overlapping pair (i < j) of a session's stored keyframes with the robust alignment - template image i, other image j, start composed from the two
 * matrices - and solves for all their places at once: per entry k of the anchor's component a correction delta_k (four-corner offsets in keyframe k's
 * own pixels, X_k' = H(delta_k) . X_k), by Levenberg-Marquardt on sum r^T W r over the accepted edges, r = offsets - corners(H(delta_j) X_j X_i^-1
 * H(delta_i)^-1).  The anchor - the usable entry with the fewest links, then the lowest slot - does not move.  All or nothing per session: the new
 * matrices exist only under HNET_ADJ_ADJUSTED.  Opt-in: a sessions object that never calls hnet_sessions_enable_keyframe_adjust allocates, launches and
 * returns what it did. */
enum { HNET_ADJ_FEW_ENTRIES = 1,       /* fewer than two usable (valid, invertible) entries */
       HNET_ADJ_NO_EDGES = 2,          /* no accepted edge reaches the anchor */
       HNET_ADJ_SINGULAR = 4,          /* the normal matrix has a Cholesky pivot <= 1e-12 max diag, or a step is not finite: the edges leave an entry free */
       HNET_ADJ_NO_GAIN = 8,           /* not cost < cost0 */
       HNET_ADJ_SHIFT_ABOVE_MAX = 16,  /* max_shift_px > 0 and the worst |delta| exceeds it: the guard against a false match */
       HNET_ADJ_CHAIN = 32,            /* a H(delta_k) . X_k is degenerate */
       HNET_ADJ_ADJUSTED = 64,         /* the record's h_origin_key are the new matrices (and, with apply, the map's) */
       HNET_ADJ_CONVERGED = 128 };     /* beside the verdict: an accepted step moved no component by eps_px or more */
enum { HNET_ADJ_EDGE_ACCEPTED = 1, HNET_ADJ_EDGE_STOPPED = 2, HNET_ADJ_EDGE_MSE_ABOVE_MAX = 4, HNET_ADJ_EDGE_NON_FINITE = 8, HNET_ADJ_EDGE_LOW_OVERLAP = 16,
       HNET_ADJ_EDGE_CLOSURE_ABOVE_MAX = 32,   /* hnet_keyframe_revisit's reasons, in its order */
       HNET_ADJ_EDGE_NO_RELATIVE = 64 };       /* a caller-supplied row that cannot be an edge: slots not i < j < m, an unusable endpoint, a non-finite offset */
enum { HNET_ADJ_WEIGHT_UNIT = 0,       /* W = I */
       HNET_ADJ_WEIGHT_INFO = 1 };     /* W = the record's 8 x 8 information matrix / max(mse, mse_floor) */
#define HNET_ADJ_MAX_EDGES 28
#define HNET_ADJ_MAX_TRIALS 64
typedef struct hnet_keyframe_adjust_opts {
    hnet_photo_robust_opts align;      /* the alignment of every pair */
    int32_t levels, min_grid;          /* its levels (1 .. 4); the fewest grid points (of 64) of keyframe i inside keyframe j for a pair to be a job */
    double  min_overlap, max_mse, max_closure_px;      /* an edge's gates, as hnet_keyframe_revisit_opts' (0: no limit, the last two) */
    int32_t weighting, max_trials;     /* HNET_ADJ_WEIGHT_*; trials of the solve at the most, 1 .. HNET_ADJ_MAX_TRIALS */
    double  mse_floor, lambda0, eps_px, max_shift_px;  /* the floor under an edge's mse (> 0); initial damping (0 < . <= 1e100); convergence (px); 0: no limit */
    int32_t apply, pad;                /* 1: the new matrices are written into the map (the operator-level calls have no map: ignored there) */
} hnet_keyframe_adjust_opts;
typedef struct hnet_keyframe_adjust_edge {
    int32_t i, j, grid, flags;         /* the pair, keyframe i's grid count inside j, HNET_ADJ_EDGE_* */
    float   start_px[8], offsets_px[8];/* the alignment's start and result: where keyframe i's corners lie in j */
    double  mse, overlap;              /* the record's mean robust cost and n_valid / 71 680 */
    double  r0_px, r_px;               /* the worst residual component before and after the solve (0 for an edge outside it) */
} hnet_keyframe_adjust_edge;
typedef struct hnet_keyframe_adjust {
    int32_t flags, anchor;             /* HNET_ADJ_*; the anchor's slot or -1 */
    int32_t n_pairs, n_jobs, n_edges;  /* pairs of usable entries, those aligned, those accepted */
    int32_t adjusted_mask, unconnected_mask;   /* the anchor's component (the anchor included); the usable entries outside it, which keep their bytes */
    int32_t trials, accepted, pad;
    double  cost0, cost, lambda;
    double  delta_px[8][8];            /* what the solve reached, whenever it ran (zeros for the anchor and outside the component) */
    double  h_origin_key[8][9];        /* under HNET_ADJ_ADJUSTED the new matrices; the old one for every other slot below the capacity, zeros above */
    hnet_keyframe_adjust_edge edge[HNET_ADJ_MAX_EDGES];        /* the jobs in pair order; unused rows are zero */
} hnet_keyframe_adjust;                /* every byte written: records compare byte for byte */
void hnet_keyframe_adjust_default_opts(hnet_keyframe_adjust_opts* o);
/* Operator level, the solve alone: caller-supplied entries [m] (1 .. 8) and edge rows [n_edges] (0 .. 28; i, j, flags, offsets_px and mse are read),
 * edge_infos NULL (identity) or [n_edges][64], as one session of capacity m.  One upload, one launch, one download, one synchronisation.
 * HNET_ERR_INVALID_ARG, nothing written: a null argument, m or n_edges out of range, invalid options. */
int  hnet_op_keyframe_adjust_solve(hnet_ctx* ctx, int m, const hnet_keyframe_map_entry* entries, int n_edges, const hnet_keyframe_adjust_edge* edges,
                                   const double* edge_infos, const hnet_keyframe_adjust_opts* opts, hnet_keyframe_adjust* out);
/* Operator level, the whole adjustment: pairs, alignments and solve on caller-supplied images [m][224][320] and entries [m].  out_edge_records NULL or
 * [28] level-0 records of the jobs, in job order (unused rows zero).  The jobs run in rounds of max_batch alignments; TWO synchronisations, one after the
 * pairs (a small download of the job table sizes the rounds) and one at the end.  Errors as above. */
int  hnet_op_keyframe_adjust(hnet_ctx* ctx, int m, const uint8_t* images, const hnet_keyframe_map_entry* entries, const hnet_keyframe_adjust_opts* opts,
                             hnet_keyframe_adjust* out, hnet_photo_robust* out_edge_records);
/* once, after hnet_sessions_enable_keyframe_map: job tables, edge tables, records, pinned blocks and events of max_batch slots.
 * HNET_ERR_INVALID_ARG: before the map, a second call. */
int  hnet_sessions_enable_keyframe_adjust(hnet_sessions* s);
/* The listed sessions' maps, each adjusted on its own: out [n], out_edge_records NULL or [n][28].  An occasional call after a closure, not a per-tick
 * one: the jobs of all listed sessions run in rounds of max_batch alignments (a session's jobs may straddle a round) on the staging arrays and the
 * alignment scratch of the keyframe store, and the call has TWO synchronisations, one after the pairs kernel and one at the end.
 * hnet_sessions_last_keyframe_device_ms covers it (from the pairs kernel to the solve, the host's sizing of the rounds included).  With opts.apply the
 * new matrices are written into the map's entries and the state's h_origin_key follows entry cur_slot's; valid, links, serial, cursor, key_px, age and
 * the images are never touched; without it the call is read-only.  A session with fewer than two valid entries is not an error: HNET_ADJ_FEW_ENTRIES.
 * Refused before anything is enqueued, nothing written: HNET_ERR_INVALID_ARG for a call before the enable, a null argument, invalid options, an id out
 * of range or repeated; HNET_ERR_CAPACITY for n > max_batch. */
int  hnet_sessions_keyframe_adjust(hnet_sessions* s, int n, const int32_t* ids, const hnet_keyframe_adjust_opts* opts, hnet_keyframe_adjust* out,
                                   hnet_photo_robust* out_edge_records);

int hnet_synchronize(hnet_ctx* ctx, void* stream);
int hnet_last_timing(const hnet_ctx* ctx, hnet_timing* out);

/* Device-time measurement of `iters` back-to-back forwards on resident buffers (HIP events on the
 * context's stream).  per_iter_ms may be NULL.  Used by bench.py for latency percentiles. */
int hnet_time_batch_device(hnet_ctx* ctx, const void* d_prev, const void* d_curr, int pix_fmt,
                           const float* d_prior, int batch, uint64_t pair_seq0, float* d_mean, float* d_cov,
                           int iters, float* per_iter_ms, float* total_ms);

/* Per-stage device timing: a "stage" is one kernel launch of the forward (prep / conv layer / fc+DLT / heads).
 * hnet_profile_batch_device runs `iters` forwards with a HIP event after every launch on the context's stream
 * and returns the average milliseconds per stage ([hnet_stage_count] floats).  flops_per_pair = 2 x MACs.  The stage list is that of a
 * forward of max_batch pairs until a profile call names another batch: batches <= 8 take the latency path, which has fewer launches
 * (never more than the max_batch list), and hnet_stage_count / _name then describe the batch last profiled. */
int hnet_stage_count(const hnet_ctx* ctx);
const char* hnet_stage_name(const hnet_ctx* ctx, int i);
double hnet_stage_flops_per_pair(const hnet_ctx* ctx, int i);
/* kernels the stage's launch consisted of in the last profiled forward (a split-K layer with a separate reduce launch: 2); the fp32-MFMA mode reports 1 */
int hnet_stage_kernels(const hnet_ctx* ctx, int i);
int hnet_profile_batch_device(hnet_ctx* ctx, const void* d_prev, const void* d_curr, int pix_fmt,
                              const float* d_prior, int batch, uint64_t pair_seq0, float* d_mean, float* d_cov,
                              int iters, float* stage_ms_avg);

/* ---- operator-level entry points (parity tests of single kernels; host buffers, NCHW like the reference) ---- */

/* warp.py:60-79 — img [224][320] float32, H[9] -> out [224][320] */
int hnet_op_warp(hnet_ctx* ctx, const float* img, const float* H, float* out);
/* model_to_trace.py:42-61 — dst corners [n][8] -> H [n][9] */
int hnet_op_dlt(hnet_ctx* ctx, const float* dst, int n, float* H);
/* conv layer `layer` (0..19, execution order of cuahn_vio_amd/weights.py CONV_LAYERS) with its own weights:
 * in [B][Cin][H][W] -> out [B][Cout][Ho][Wo], + bias + LeakyReLU(0.1)   (model_to_trace.py:7-15) */
int hnet_op_conv(hnet_ctx* ctx, int layer, const float* in, int batch, int h, int w, float* out);
/* the fused block_4_0 + block_4_1 kernel of the split-bf16 mode (csrc/conv_b4_fused.h) on its own:
 * in [B][2][224][320] -> out [B][16][112][160] = conv_lrelu(conv_lrelu(in, block_4_0), block_4_1)   (model_to_trace.py:210-211).
 * reverse != 0 walks the tiles from the end of the batch.  HNET_ERR_UNSUPPORTED in the other arithmetic modes. */
int hnet_op_block4_fused(hnet_ctx* ctx, const float* in, int batch, int reverse, float* out);
/* the fused block_3_0 + block_3_1 kernel alone (fp16-plane mode): in [B][2][112][160] (NCHW fp32) -> out [B][32][56][80] = conv(conv(in)) with
 * the reference's conv() (model_to_trace.py:7-15, layers :108-109) */
int hnet_op_block3_fused(hnet_ctx* ctx, const float* in, int batch, float* out);
/* the fused block_4_2 + block_4_3 kernel alone (fp16-plane mode): in [B][16][112][160] -> out [B][64][28][40] (model_to_trace.py:212-213) */
int hnet_op_block42_fused(hnet_ctx* ctx, const float* in, int batch, float* out);
/* cat(img1, warp(img2,H)) -> AvgPool(k): img1,img2 [224][320] f32, H[9] or NULL (no warp), k in {1,2,4,8}
 * -> out [2][224/k][320/k]   (model_to_trace.py:153-157) */
int hnet_op_prep(hnet_ctx* ctx, const float* img1, const float* img2, const float* H, int k, float* out);
/* the same on u8 images as load_current_img receives them (u8 -> f32 / 255.0, HomographyNet.cpp:139-146) */
int hnet_op_prep_u8(hnet_ctx* ctx, const uint8_t* img1, const uint8_t* img2, const float* H, int k, float* out);
/* the same for n pairs in ONE launch, as the forward issues it: img1, img2 [n][224][320] of pix_fmt (HNET_PIX_*), H [n][9] or NULL, the context's sampler
 * (hnet_config.warp_exact) -> out [n][2][224/k][320/k].  The frames are uploaded to device addresses align_off bytes (0 .. 15; a multiple of 4 for float
 * frames) past a 16-byte boundary: 0 takes the tiled kernels, anything else the routes of frames that are not 16-byte aligned.
 * planes != NULL (k = 1 with H; HNET_ERR_UNSUPPORTED on a context whose forward has no block-4 plane input): the launch writes the block-4 input as the
 * forward's 16-bit planes (two fp16 planes in HNET_PREC_F16X2, three bf16 planes in HNET_PREC_BF16X3, one in HNET_PREC_BF16) into a buffer filled with
 * 0xA5A5A5A5; planes receives its dwords [n_planes][n][235][336] (pixel (u, v) at row v + 5, column u + 5; low half img1, high half the warped img2) and
 * out the values the planes join to. */
int hnet_op_prep_batch(hnet_ctx* ctx, const void* img1, const void* img2, int pix_fmt, const float* H, int n, int k, int align_off, float* out,
                       uint32_t* planes);
/* after a forward: copies the output of layer `layer` (0..19 convs) of pair `pair` as [Cout][Ho][Wo] */
int hnet_debug_layer_output(hnet_ctx* ctx, int layer, int pair, float* out, size_t capacity_floats);
/* after a forward: part-1 homography of pair `pair`, 9 floats */
int hnet_debug_h_part1(hnet_ctx* ctx, int pair, float* out9);

#ifdef __cplusplus
}
#endif
#endif /* HNET_H */
