/*
 * rsx.h -- C-ABI of librsx.so: the MI355X-native (gfx950, HIP) ScanContext + ORORA hot path of
 * navtech-radar-slam.  Plain pointers and sizes only; no C++/torch types cross this boundary.
 *
 * Reference interfaces each group replaces (paths under the reference checkout):
 *   SC  = pgo/SC-A-LOAM/include/scancontext/Scancontext.{h,cpp}
 *   PGO = pgo/SC-A-LOAM/src/laserPosegraphOptimization.cpp
 *
 * Conventions
 *   - every function returns an rsx_status (0 = ok, <0 = error); a loop id of -1 is DATA ("no
 *     loop", SC.cpp:333), not an error.  No C++ exception crosses the ABI.
 *     rsx_last_error_string() gives a thread-local diagnostic.
 *   - the caller owns every buffer it passes; the library copies inputs before returning and
 *     writes outputs into caller memory.  Pointers named d_* are DEVICE (HBM) pointers of the
 *     handle's GPU and are used asynchronously on the given hipStream_t (passed as void*).
 *     A NULL stream selects the handle's own private (non-blocking) stream, NOT the legacy default
 *     stream: callers that mix several handles or other GPU work must pass one explicit stream.
 *     (The rsx_sc device entries start a NULL-stream call behind what the legacy default stream holds at the call, so that
 *     buffers a framework filled on its default stream are complete; nothing orders the legacy stream behind the library.)
 *     Calls on ONE handle that pass different streams are ordered by the library (the handle's workspaces are shared: a call
 *     arriving on another stream than the previous call makes its stream wait for everything enqueued on the old one).
 *     The one exemption is rsx_ransac_estimate_batch_device, which uses no workspace of its handle.
 *   - a handle is internally synchronised: every entry point holds the handle's mutex for its whole
 *     duration, so any number of threads may call concurrently (the reference itself races between its
 *     writer, PGO.cpp:492 process_pg, and its reader, PGO.cpp:561 process_lcd).  The one multi-call
 *     protocol, query stage 1 -> stage 2, is invalidated (stage 2 fails with RSX_ERR_BAD_ARG) by any
 *     other query-type call on the same handle in between, instead of reading clobbered workspaces.
 *   - there is NO CPU fallback: without a usable HIP device rsx_*_create fails with
 *     RSX_ERR_NO_DEVICE.
 *
 * Descriptor layouts
 *   - "colmajor double": 20 x 60 Eigen::MatrixXd memory order (SC.cpp:159), element
 *     (ring r, sector s) at [s*20 + r]; 9600 B.
 *   - "f32 sector-major": the same order in float, 4800 B; every descriptor the reference can
 *     build is exactly representable in fp32 (SC.cpp:168: pt.z is a float).
 */
#ifndef RSX_H
#define RSX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSX_SC_NUM_RING 20    /* SC.h:85  PC_NUM_RING   */
#define RSX_SC_NUM_SECTOR 60  /* SC.h:86  PC_NUM_SECTOR */
#define RSX_SC_DESC_SIZE 1200
#define RSX_SC_MAX_TOPK 32

typedef enum {
  RSX_OK = 0,
  RSX_ERR_BAD_ARG = -1,
  RSX_ERR_NO_DEVICE = -2,
  RSX_ERR_HIP = -3,
  RSX_ERR_OOM = -4,
  RSX_ERR_NOT_FP32_EXACT = -5, /* a colmajor-double descriptor does not round-trip through fp32 */
  RSX_ERR_RANGE = -6,
  RSX_ERR_INTERNAL = -7
} rsx_status;

const char *rsx_last_error_string(void);
/* "rsx <version> gfx950 ..." */
const char *rsx_version(void);
/* number of visible HIP devices (0 on a box without a GPU; never an error) */
int rsx_device_count(void);

/* ============================== ScanContext (SC.h:62-122) ============================== */

typedef struct rsx_sc rsx_sc; /* replaces a `SCManager` instance (PGO.cpp:99) */

/* one loop candidate: distanceBtnScanContext() result (SC.cpp:116-148) + DB index */
typedef struct {
  double dist;   /* min over the searched column shifts of the mean column cosine distance */
  int32_t index; /* GLOBAL keyframe index */
  int32_t shift; /* argmin column shift; yaw = shift * 6 deg */
} rsx_sc_hit;

typedef struct {
  double lidar_height;        /* SC.h:83  LIDAR_HEIGHT = 2.0 */
  double max_radius;          /* SC.h:87  PC_MAX_RADIUS = 80 */
  int32_t num_exclude_recent; /* SC.h:92  = 30 */
  int32_t num_candidates;     /* SC.h:93  NUM_CANDIDATES_FROM_TREE = 3 (<= 32) */
  double search_ratio;        /* SC.h:96  = 0.1 (kernels are specialised for the resulting +-3 window) */
  double dist_thres;          /* SC.h:99  SC_DIST_THRES = 0.2 (sc_pgo.launch:4 sets 0.45) */
  int32_t tree_making_period; /* SC.h:103 = 30 */
  int32_t device;             /* HIP device ordinal */
  /* DB sharding over GPUs: this handle stores the entries whose global index i has
   * i % shard_world == shard_rank (block-cyclic), local slot i / shard_world. */
  int32_t shard_rank;         /* default 0 */
  int32_t shard_world;        /* default 1 */
  int64_t capacity_hint;      /* initial DB capacity in entries (grows by doubling) */
  /* exhaustive queries: 0 = auto (up to 16 queries per call -- the live detector asks one, PGO.cpp:561,577 -- take the
   * one-launch single-query path, sc_q1.hip; batched queries go through the MFMA lower-bound filter and only
   * the entries that can still reach the top-k are scored by the exact fp64 kernel), 1 = always
   * score every entry exactly, 2 = always the batched filter chain, 3 = the single-query path wherever it applies (<= 16
   * queries per call; auto otherwise).  Results are identical in every mode. */
  int32_t filter_mode;
  /* which form of the filter: 0 = default (3: spectral), 1 = direct (60-shift correlation as one K = 1200 MFMA GEMM per
   * shift), 3 = spectral (Z15 DFT + direct Z4 correlation, ~6x fewer MFMAs; two waves per SIMD, the entry tile split by
   * frequency over a wave pair), 2 = a synonym of 3, kept for callers: it named the spectral kernel with one wave per SIMD,
   * which gave the same bounds bit for bit and is gone.  All give valid lower bounds of the same quantity; results are
   * identical. */
  int32_t filter_kind;
  /* summation order of the sums the reference takes through Eigen (mean, norm, dot): a property of how the REFERENCE was
   * built, which the bit-exact contract follows.  RSX_SC_SUM_EIGEN_SSE2 (0, default) = the reference as its CMakeLists.txt
   * builds it (x86-64, -O3, 2-double packets); RSX_SC_SUM_SEQ = Eigen without vectorisation; RSX_SC_SUM_EIGEN_AVX_FMA = a
   * workspace compiled with -march=native (4-double packets, fused multiply-adds).  csrc/sc_redux_dev.h. */
  int32_t sum_order;
} rsx_sc_params;
#define RSX_SC_SUM_EIGEN_SSE2 0
#define RSX_SC_SUM_SEQ 1
#define RSX_SC_SUM_EIGEN_AVX_FMA 2
#define RSX_SC_SUM_EIGEN34_AVX_FMA 3 /* as 2 against Eigen 3.4: its AVX horizontal add is (l0 + l2) + (l1 + l3), 3.3's (l0 + l1) + (l2 + l3) */

typedef enum {
  RSX_SC_MODE_CANDIDATE = 0, /* reference semantics: ring-key 3-NN then 3 pair distances (SC.cpp:331-422) */
  RSX_SC_MODE_EXHAUSTIVE = 1 /* same pair function against every eligible entry */
} rsx_sc_mode;


int rsx_sc_default_params(rsx_sc_params *p);
int rsx_sc_create(const rsx_sc_params *p, rsx_sc **out);   /* SCManager() */
int rsx_sc_destroy(rsx_sc *h);
int rsx_sc_set_dist_thres(rsx_sc *h, double thres);        /* setSCdistThres, SC.cpp:262-265 */
/* number of keyframes known to this handle (GLOBAL count; a shard stores ~1/world of them) */
int rsx_sc_size(rsx_sc *h, int64_t *n_global);
int rsx_sc_local_size(rsx_sc *h, int64_t *n_local);

/* makeAndSaveScancontextAndKeys (SC.cpp:249-260).  pts: n points, stride_bytes apart
 * (32 for pcl::PointXYZI), float x,y,z at byte offsets 0,4,8.  The descriptor, ring key, sector
 * key and column norms are built on the GPU.  In a sharded handle every rank must call this for
 * every keyframe (same order); ranks that do not own the slot only advance the global count.
 * out_index (optional) = global index of the new keyframe.
 * The call copies the cloud (pts is free again on return) and enqueues ONE kernel; it does not wait for the GPU.  Every
 * later call on the handle sees the entry (calls that bring their own stream are ordered behind it); a device fault of
 * the insert is reported by the next call that synchronises. */
int rsx_sc_add_points(rsx_sc *h, const void *pts, size_t n, size_t stride_bytes, int32_t *out_index);
/* saveScancontextAndKeys (SC.cpp:236-246), colmajor double; RSX_ERR_NOT_FP32_EXACT if lossy */
int rsx_sc_add_descriptor(rsx_sc *h, const double *desc_colmajor, int32_t *out_index);
/* the same for descriptors that did not come out of makeScancontext (e.g. SCDs re-read from decimal text
 * files in multi-session use): every element is rounded to fp32 -- the DB stores fp32 -- and the largest
 * absolute rounding error is reported (optional).  NaN elements are still rejected. */
int rsx_sc_add_descriptor_rounded(rsx_sc *h, const double *desc_colmajor, int32_t *out_index, double *max_abs_rounding);
/* bulk import of n f32 sector-major descriptors (host memory); same sharding rule */
int rsx_sc_add_descriptors_f32(rsx_sc *h, const float *descs, int64_t n);
/* the same from DEVICE memory (no host round trip), n consecutive global keyframes */
int rsx_sc_add_descriptors_f32_device(rsx_sc *h, const float *d_descs, int64_t n, void *stream);

/* bulk export: the f32 sector-major descriptors of LOCAL slots [first_slot, first_slot + count) (host out) */
int rsx_sc_export_descriptors_f32(rsx_sc *h, int64_t first_slot, int64_t count, float *out);
/* on-disk database (the re-ingest side is saveScancontextAndKeys, SC.cpp:236-246): a 64-byte
 * little-endian header {"RSXSCDB1", version, rings, sectors, dtype, n_global, n_local, shard_rank, shard_world}
 * followed by the handle's n_local fp32 sector-major descriptors.  Keys, norms and filter images are rebuilt on the
 * GPU by rsx_sc_load.  An unsharded file appends to any handle (each shard keeps its residue class); a shard file
 * restores that shard into an empty handle with the same shard_rank / shard_world. */
int rsx_sc_save(rsx_sc *h, const char *path);
int rsx_sc_load(rsx_sc *h, const char *path, int64_t *n_loaded);

/* polarcontexts_[i] / getConstRefRecentSCD (SC.h:79,111): global index must be owned by this shard */
int rsx_sc_get_descriptor(rsx_sc *h, int64_t index, double *out_colmajor);
int rsx_sc_get_ringkey(rsx_sc *h, int64_t index, float *out20);     /* polarcontext_invkeys_mat_ */
int rsx_sc_get_sectorkey(rsx_sc *h, int64_t index, double *out60);  /* polarcontext_vkeys_ */

/* detectLoopClosureID (SC.cpp:331-422).  loop_id/-1 and yaw are the reference's return pair;
 * min_dist / nn_idx (optional) are the values of its log line (SC.cpp:406,412).
 * mode CANDIDATE reproduces the reference (frozen searchable prefix rebuilt every
 * tree_making_period calls, NUM_EXCLUDE_RECENT, kNN order, strict-< first-wins);
 * mode EXHAUSTIVE scores the whole frozen prefix.  Unsharded handles only. */
int rsx_sc_detect_loop_closure(rsx_sc *h, int mode, int32_t *loop_id, float *yaw_diff_rad,
                               double *min_dist, int32_t *nn_idx);
/* the same with everything the reference's log line shows (SC.cpp:406,412: "[Loop found] Nearest distance: <min_dist>
 * btn <query_idx> and <nn_idx>."), taken under one lock so that query_idx is the keyframe that was actually the query */
typedef struct {
  int32_t loop_id;      /* nn_idx if min_dist < dist_thres else -1 */
  float yaw_diff_rad;
  double min_dist;
  int32_t nn_idx;
  int32_t query_idx;    /* polarcontexts_.size() - 1 at the time of the call */
  int32_t searched;     /* 0: the early return of SC.cpp:341-345 (fewer than NUM_EXCLUDE_RECENT + 1 keyframes; the
                           reference prints nothing then) */
  int32_t reserved;
  double dist_thres;    /* the threshold that was applied */
} rsx_sc_detection;
int rsx_sc_detect_loop_closure_ex(rsx_sc *h, int mode, rsx_sc_detection *out);
/* detectLoopClosureIDBetweenSession (SC.cpp:267-328): query passed in, tree over the whole DB
 * as of the first call. */
int rsx_sc_detect_between_session(rsx_sc *h, const float *curr_key20, const double *curr_desc_colmajor,
                                  int32_t *loop_id, float *yaw_diff_rad, double *min_dist,
                                  int32_t *nn_idx);
/* current frozen searchable prefix length ("tree" size, SC.cpp:352-353) */
int rsx_sc_tree_size(rsx_sc *h, int64_t *n);

/* The reference's public helper methods (SC.h:60-66), stateless: the handle only lends its device, stream and
 * staging memory.  They run on the GPU in fp64 on the doubles as given (no fp32 storage involved, any MatrixXd
 * content is accepted) and equal the reference bit for bit.  One small launch per call: API completeness, not
 * the batched path.
 *   makeScancontext (SC.cpp:151-195)                          -> 20 x 60 colmajor double */
int rsx_sc_make_scancontext(rsx_sc *h, const void *pts, size_t n, size_t stride_bytes, double *out_desc_colmajor);
/*   makeRingkeyFromScancontext / makeSectorkeyFromScancontext (SC.cpp:198-227), either output optional */
int rsx_sc_make_keys(rsx_sc *h, const double *desc_colmajor, double *out_ringkey20, double *out_sectorkey60);
/*   distDirectSC (SC.cpp:69-90): no alignment, no shift; NaN when no column is effective */
int rsx_sc_dist_direct(rsx_sc *h, const double *sc1_colmajor, const double *sc2_colmajor, double *out_dist);
/*   fastAlignUsingVkey (SC.cpp:93-113) on two 1 x 60 sector keys */
int rsx_sc_fast_align(rsx_sc *h, const double *vkey1_60, const double *vkey2_60, int32_t *out_shift);
/*   distanceBtnScanContext (SC.cpp:116-148) */
int rsx_sc_distance(rsx_sc *h, const double *sc1_colmajor, const double *sc2_colmajor, double *out_dist, int32_t *out_shift);

/* Exhaustive batched query (the north-star path): nq f32 sector-major query descriptors against
 * every LOCAL entry whose global index < n_eligible (n_eligible < 0: all); out = nq x k records
 * sorted by (dist, index), padded with {1e7, 0, 0} (SC.cpp:362-364 initial values).
 * Host-buffer form (synchronous): */
int rsx_sc_query(rsx_sc *h, const float *q_descs, int32_t nq, int32_t k, int64_t n_eligible,
                 rsx_sc_hit *out);
/* Device-buffer form: asynchronous on `stream` (hipStream_t); d_out stays on the GPU so a sharded
 * caller can all-gather it (RCCL) without a host hop. */
int rsx_sc_query_device(rsx_sc *h, const float *d_q_descs, int32_t nq, int32_t k, int64_t n_eligible,
                        rsx_sc_hit *d_out, void *stream);
/* Filter shards over a REPLICATED database (the layout that scales when the batch is large and the DB small
 * next to HBM: 1.43 GB per 100 000 keyframes -- 14 308 B each, 960 B of them the packed columns).  Every rank holds every keyframe (shard_world 1); only the lower-bound
 * filter -- the per-pair cost -- is cut over the ranks by slot range, the per-query stages (short list, window previews,
 * exact re-scoring) run on each rank for ITS slice of the batch against the whole DB:
 *   every rank r   rsx_sc_filter_range_device: all nq queries x slots [first_r, first_r + n_r)  -> d_lb[nq][ld_r]
 *   caller         all-to-all of the row slices (RCCL): rank t receives rows [q_t, q_t + nq_t) of every rank's matrix,
 *                  one column block per sender
 *   every rank t   rsx_sc_query_bounds_device: its nq_t queries with the received column blocks -> d_out[nq_t][k]
 *   caller         all-gather of d_out
 * The records are those of rsx_sc_query_device on one GPU (the bounds of a pair do not depend on who computed them).
 * first_slot must be a multiple of 32 (the filter images are stored in tiles of 32 entries); d_lb[q * ld + j] is the bound
 * of query q against slot first_slot + j, ld >= n_slots rounded up to 32 (columns past n_slots are unspecified).
 * Bounds are IEEE binary16 (rsx_f16), rounded toward zero -- the element type of the library's own bound matrix.
 * d_lb and d_lb_blocks must be 16-byte aligned (RSX_ERR_BAD_ARG otherwise: they are written / read with 16-byte accesses).
 * n_slots == 0 is a no-op whatever first_slot says (a rank whose range lies beyond the entries of a small database). */
typedef uint16_t rsx_f16;
int rsx_sc_filter_range_device(rsx_sc *h, const float *d_q_descs, int32_t nq, int64_t first_slot, int64_t n_slots,
                               rsx_f16 *d_lb, int64_t ld, void *stream);
/* d_lb_blocks: n_blocks column blocks, block b = [nq][block_ld] bounds starting b * block_stride elements (a multiple of 8)
 * into the buffer,
 * its column j = the bound against slot b * block_ld + j (block_ld a multiple of 32; the blocks together must cover every
 * entry below n_eligible).  Scores nq queries exactly like rsx_sc_query_device, with these bounds in place of its own
 * filter launch. */
int rsx_sc_query_bounds_device(rsx_sc *h, const float *d_q_descs, int32_t nq, int32_t k, int64_t n_eligible,
                               const rsx_f16 *d_lb_blocks, int32_t n_blocks, int64_t block_ld, int64_t block_stride,
                               rsx_sc_hit *d_out, void *stream);
/* The same query in two stages, for a DB sharded over several GPUs.  With one stage
 * every shard would have to re-score the entries that look promising against ITS OWN k-th best
 * distance; with two, the shards first agree on a global bound:
 *   stage 1  filter + this shard's share of the lowest-bound entries   -> d_partial[nq][k]
 *   caller   all-gather d_partial over the ranks (RCCL), rsx_sc_merge_topk_device -> d_global[nq][k]
 *   stage 2  only entries whose bound can still beat the k-th distance of d_global are scored;
 *            d_out[nq][k] = this shard's top-k including its stage-1 hits
 *   caller   all-gather d_out, rsx_sc_merge_topk_device -> the global top-k
 * d_q_descs must stay valid until stage 2 has run; stage 2 must follow stage 1 on the same handle
 * with the same nq and k.  The merged result is identical to rsx_sc_query_device + merge. */
int rsx_sc_query_stage1_device(rsx_sc *h, const float *d_q_descs, int32_t nq, int32_t k, int64_t n_eligible,
                               rsx_sc_hit *d_partial, void *stream);
/* the same with a per-query eligibility limit (device array, nq entries): query i only sees entries
 * with global index < min(n_eligible, d_q_elig[i]) -- e.g. "every keyframe against the keyframes at
 * least 30 older than itself" over a sharded DB (BASELINE configs 4 and 5).  elig_monotone != 0
 * promises that d_q_elig does not decrease with i, which lets the filter skip the tile-blocks a
 * query cannot see.  d_q_elig must stay valid until stage 2 has run. */
int rsx_sc_query_stage1_elig_device(rsx_sc *h, const float *d_q_descs, int32_t nq, int32_t k, int64_t n_eligible,
                                    const int64_t *d_q_elig, int32_t elig_monotone, rsx_sc_hit *d_partial,
                                    void *stream);
int rsx_sc_query_stage2_device(rsx_sc *h, int32_t nq, int32_t k, const rsx_sc_hit *d_global, rsx_sc_hit *d_out,
                               void *stream);
/* queries = DB entries [q_first, q_first+nq) of this handle (all-pairs runs, BASELINE config 5);
 * each query i uses n_eligible = min(n_eligible, q_first+i - exclude_recent) when exclude_recent >= 0 */
int rsx_sc_query_self_device(rsx_sc *h, int64_t q_first, int32_t nq, int32_t k, int64_t n_eligible,
                             int32_t exclude_recent, rsx_sc_hit *d_out, void *stream);
/* parity helper: dist/shift of ONE query against local entries [first, first+count) (host out) */
int rsx_sc_pair_distances(rsx_sc *h, const float *q_desc, int64_t first, int64_t count,
                          double *out_dist, int32_t *out_shift);
/* merge nparts per-shard top-k lists (layout [part][nq][k]) into out[nq][k]; pure host logic */
int rsx_sc_merge_topk(const rsx_sc_hit *parts, int32_t nparts, int32_t nq, int32_t k, rsx_sc_hit *out);
/* the same on the GPU (d_parts is what an RCCL all-gather of d_out produces) */
int rsx_sc_merge_topk_device(rsx_sc *h, const rsx_sc_hit *d_parts, int32_t nparts, int32_t nq,
                             int32_t k, rsx_sc_hit *d_out, void *stream);
/* apply the loop threshold + yaw conversion of SC.cpp:401-417 to a top-1 record */
int rsx_sc_hit_to_loop(rsx_sc *h, const rsx_sc_hit *hit, int32_t *loop_id, float *yaw_diff_rad);

/* ---- one process, several GPUs (SURVEY 8e for a single C++ host such as alaserPGO, PGO.cpp:99,706-710) ----
 * rsx_scs = a ScanContext database sharded over the listed devices (keyframe i on shard i % n_devices), driven
 * by the calling process: one stream per device, the two-stage query above with the exchanges done as peer
 * copies over xGMI.  Results are identical to an unsharded handle.  The same device may be listed more than once
 * (several shards on one GPU: used by the tests on one-GPU boxes).  Internally synchronised. */
typedef struct rsx_scs rsx_scs;
int rsx_scs_create(const rsx_sc_params *p, const int32_t *devices, int32_t n_devices, rsx_scs **out);
/* The general form.  Layout: n_devices = query_groups x DB shards; device g belongs to query group g / S and holds DB
 * shard g % S (S = n_devices / query_groups; keyframe i on the shards i % S, once per group).  A batch is cut into
 * query_groups contiguous slices, each answered by its group: per-query costs shrink with the number of groups, per-pair
 * costs with the number of devices (rsx_scs_create = 1 group: every device a shard of ONE database copy).
 * exchange_kind: how the shards of a group exchange their 16-byte records in the two-stage query --
 *   RSX_SCS_EXCHANGE_PEER_COPY  hipMemcpyPeerAsync to the group's first device and back (default; no extra library)
 *   RSX_SCS_EXCHANGE_RCCL       ncclAllGather over the group's communicators, every shard merges for itself; librccl.so is
 *                               loaded on first use (dlopen); devices inside a group must be distinct
 * Results are identical in every layout and with either exchange. */
#define RSX_SCS_EXCHANGE_PEER_COPY 0
#define RSX_SCS_EXCHANGE_RCCL 1
int rsx_scs_create_layout(const rsx_sc_params *p, const int32_t *devices, int32_t n_devices, int32_t query_groups, int32_t exchange_kind,
                          rsx_scs **out);
int rsx_scs_num_query_groups(rsx_scs *h);
int rsx_scs_destroy(rsx_scs *h);
int rsx_scs_num_shards(rsx_scs *h); /* DB shards per query group */
int rsx_scs_set_dist_thres(rsx_scs *h, double thres);
int rsx_scs_size(rsx_scs *h, int64_t *n_global);
int rsx_scs_add_points(rsx_scs *h, const void *pts, size_t n, size_t stride_bytes, int32_t *out_index);
int rsx_scs_add_descriptors_f32(rsx_scs *h, const float *descs, int64_t n);
int rsx_scs_get_descriptor(rsx_scs *h, int64_t index, double *out_colmajor);
/* exhaustive batched query, host buffers in and out (synchronous); same contract as rsx_sc_query */
int rsx_scs_query(rsx_scs *h, const float *q_descs, int32_t nq, int32_t k, int64_t n_eligible, rsx_sc_hit *out);
/* detectLoopClosureID over the sharded database in EXHAUSTIVE mode (frozen prefix, 30-exclusion, threshold and yaw
 * as the reference; every entry of the prefix scored) */
int rsx_scs_detect_loop_closure(rsx_scs *h, rsx_sc_detection *out);


/* ============================== ORORA registration ======================================
 * Replaces the solver stage of the upstream file-based `odometry.cpp` entry (reference
 * README.md:27; package `orora`, launch/navtech_radar_slam_mulran.launch:5-8).  The ORORA sources
 * are an empty submodule in the reference checkout (.gitmodules:1-3), so these entry points follow
 * the published algorithm (oracle/orora_ref.h) -- parity unpinned.
 * Stateless per call; a handle only owns a stream and staging buffers. */

typedef struct rsx_orora rsx_orora;

typedef struct {
  double tim_noise_bound;        /* bound on ||b - R a|| of an inlier TIM (2 x point noise bound) */
  double noise_bound_radial;     /* A-COTE radial bound [m] */
  double noise_bound_tangential; /* A-COTE tangential bound [rad] (x range) */
  double gnc_factor;             /* mu growth per GNC iteration (1.4) */
  double cost_threshold;         /* GNC stops when |cost - prev_cost| < this */
  int32_t max_iterations;        /* GNC iteration cap */
  int32_t flags;                 /* RSX_ORORA_*: the modelling choices the (absent) upstream source would pin */
} rsx_orora_params;
#define RSX_ORORA_COMPLETE_GRAPH 1 /* rotation TIMs on all K (K-1) / 2 pairs instead of the ring of K (O(K^2) per GNC iteration) */
#define RSX_ORORA_TEASER_COST 2    /* scalar TLS cost in TEASER++'s form: unweighted residuals + sum of the outliers' bounds */
#define RSX_ORORA_PMC 4            /* max-clique inlier selection before the solver (upstream: "PMC max-clique prune"): the matches are
                                      pruned to a maximum clique of the consistency graph  i ~ j  <=>
                                      | ||src_i - src_j|| - ||dst_i - dst_j|| | < tim_noise_bound  (csrc/pmc.hip, oracle/pmc_ref.h).
                                      rsx_odometry_default_params turns it on; the device entry needs rsx_orora_reserve first */
#define RSX_ORORA_PMC_EXACT 8      /* (only with RSX_ORORA_PMC; a bad argument without it) the selection is exact: a branch-and-bound search
                                      after the greedy stage returns a MAXIMUM clique -- the greedy one where it already is one, otherwise the
                                      maximum clique first in the order (core number descending, index ascending) -- within
                                      rsx_orora_clique_node_budget() search nodes per pair.  Off by default everywhere */

typedef struct {
  double x, y, yaw;      /* dst = R(yaw) src + (x, y) */
  int32_t iterations;    /* GNC iterations executed */
  int32_t rot_inliers;   /* TIMs with final weight >= 0.5 */
  int32_t trans_inliers; /* matches inside both axis intervals at the estimate */
  int32_t status;        /* 0 ok; 1 fewer than 2 matches (identity); 2 more than
                            rsx_orora_max_correspondences() = 16384 matches (identity).  Pairs of up to 2048 matches
                            run on-chip (LDS), larger ones through an HBM workspace: same results */
} rsx_orora_result;

/* what the selection did to one pair */
typedef struct {
  int32_t size;     /* matches handed to the solver */
  int32_t max_core; /* largest core number of the consistency graph: no clique is larger than max_core + 1 */
  int32_t seeds;    /* greedy seeds started (<= 2) */
  int32_t flags;    /* RSX_ORORA_PMC_* */
} rsx_orora_pmc_info;
#define RSX_ORORA_PMC_PROVEN 1       /* size == max_core + 1: the clique is a maximum one */
#define RSX_ORORA_PMC_PASSTHROUGH 2  /* fewer than 2 or more than rsx_orora_max_clique_matches() matches: not pruned */
#define RSX_ORORA_PMC_NO_WORKSPACE 4 /* (with PASSTHROUGH) the pair did not fit what rsx_orora_reserve sized: not pruned */
#define RSX_ORORA_PMC_MAXIMUM 8      /* RSX_ORORA_PMC_EXACT: the clique is a maximum one (the search completed, or a bound proved it: set
                                        beside PROVEN as well) */
#define RSX_ORORA_PMC_BUDGET 16      /* RSX_ORORA_PMC_EXACT: the node budget ran out; the pair keeps its greedy clique */

int rsx_orora_default_params(rsx_orora_params *p);
int rsx_orora_max_correspondences(void);
int rsx_orora_max_clique_matches(void); /* 2048: pairs with more matches go to the solver unpruned */
/* Sizes the workspaces of the RSX_ORORA_PMC stage for calls of up to max_total_matches matches (sum over the pairs of a call), so
 * that the asynchronous device entry never allocates.  The host-buffer entries size them by themselves. */
int rsx_orora_reserve(rsx_orora *h, int64_t max_total_matches);
/* The selection on its own (params->tim_noise_bound is the consistency bound; NULL = defaults): out_member[m] = 1 for the
 * matches kept, laid out like the matches; out_info[n_pairs] (either may be NULL).  Host buffers, synchronous; offsets as for
 * rsx_orora_register_batch. */
int rsx_orora_max_clique_batch(rsx_orora *h, const float *src_xy, const float *dst_xy, const int64_t *offsets, int32_t n_pairs,
                               const rsx_orora_params *params, uint8_t *out_member, rsx_orora_pmc_info *out_info);
/* device buffers, asynchronous on `stream`; d_offsets are trusted (see rsx_orora_register_batch_device) */
int rsx_orora_max_clique_batch_device(rsx_orora *h, const float *d_src_xy, const float *d_dst_xy, const int64_t *d_offsets,
                                      int32_t n_pairs, const rsx_orora_params *params, uint8_t *d_member, rsx_orora_pmc_info *d_info,
                                      void *stream);
/* the info records of the last rsx_orora_register_batch{,_device} call that ran with RSX_ORORA_PMC (synchronises the handle's
 * last stream; n_pairs as in that call) */
int rsx_orora_last_pmc_info(rsx_orora *h, rsx_orora_pmc_info *out_info, int32_t n_pairs);
/* RSX_ORORA_PMC_EXACT: the search nodes one pair may cost before it keeps its greedy clique (RSX_ORORA_PMC_BUDGET); a node = one
 * branching vertex of the search.  Default 262144; nodes <= 0 is a bad argument */
int rsx_orora_set_clique_node_budget(rsx_orora *h, int64_t nodes);
int rsx_orora_clique_node_budget(rsx_orora *h, int64_t *out_nodes);
int rsx_orora_create(int device, rsx_orora **out);
int rsx_orora_destroy(rsx_orora *h);
/* n_pairs scan pairs; pair i owns matches [offsets[i], offsets[i+1]) of the concatenated
 * src_xy/dst_xy arrays (float x,y per match).  Host buffers, synchronous.  offsets[n_pairs + 1] must start at 0 and never
 * decrease: every host-buffer entry that takes offsets (this one, rsx_orora_max_clique_batch, rsx_ransac_estimate_batch,
 * rsx_mocomp_points_batch, rsx_mocomp_matches_batch) checks the whole array and refuses anything else with RSX_ERR_BAD_ARG
 * before it copies or writes anything. */
int rsx_orora_register_batch(rsx_orora *h, const float *src_xy, const float *dst_xy, const int64_t *offsets,
                             int32_t n_pairs, const rsx_orora_params *params, rsx_orora_result *out);
/* device buffers, asynchronous on `stream`.  A device entry cannot look at d_offsets: they must obey the same rule, or the
 * kernels read outside the arrays */
int rsx_orora_register_batch_device(rsx_orora *h, const float *d_src_xy, const float *d_dst_xy,
                                    const int64_t *d_offsets, int32_t n_pairs, const rsx_orora_params *params,
                                    rsx_orora_result *d_out, void *stream);

/* ============================== RANSAC / motion-compensated RANSAC ======================
 * The two other motion estimators of the upstream file-based `odometry.cpp` entry (yeti_radar_odometry's Ransac and
 * MotionDistortedRansac; Burnett et al. 2021 for the latter), beside ORORA.  Their sources are absent from the reference
 * checkout (empty submodule), so these entries follow the published methods as restated in tests/ransac_np.py, which is the
 * arithmetic contract -- parity unpinned.  2-D; no Doppler term inside the estimators (rsx_mocomp below corrects keypoints for
 * it); conventions of rsx_orora_register_batch (dst = R src + t).
 * Rigid mode: H two-match hypotheses, closed-form rigid fit, refit over the winner's inliers.  Motion-compensated mode:
 * every match carries dt = (time src was measured) - (time dst was measured) [s] and dst = exp(dt w) src for a constant
 * body velocity w = (vx, vy, wz); hypotheses and refit by Gauss-Newton.  The sampler is counter based: a pair's result
 * depends on its matches, (seed, K) and the parameters only, not on its place in the batch.  A hypothesis h is evaluated up
 * to the first one whose inlier share exceeds inlier_ratio; the one with the most inliers wins, the lowest h on a tie.
 * Stateless per call: a handle owns a stream and the staging buffers of the host-buffer entry; the device entry needs no
 * workspace, so calls on different streams neither allocate nor wait for each other. */

typedef struct rsx_ransac rsx_ransac;

typedef struct {
  double tolerance;          /* a match is an inlier when its residual is below this [m] (0.35) */
  double inlier_ratio;       /* stop at the first hypothesis with more than this share of inliers (0.90); (0, 1] */
  double gn_epsilon;         /* MC: Gauss-Newton stops when the step's norm falls below this (1e-5) */
  double dt_scan;            /* MC: the reported pose is exp(dt_scan w) (0.25 s: a Navtech head at 4 Hz) */
  int32_t max_iterations;    /* hypotheses H (100); 1 .. RSX_RANSAC_MAX_ITERATIONS */
  int32_t max_gn_iterations; /* MC: Gauss-Newton step cap (10); 1 .. 100 */
  uint64_t seed;
  int32_t flags;             /* RSX_RANSAC_* */
  int32_t reserved;
} rsx_ransac_params;
#define RSX_RANSAC_MOTION_COMPENSATED 1
#define RSX_RANSAC_MAX_ITERATIONS 1024

typedef struct {
  double x, y, yaw;      /* dst = R(yaw) src + (x, y); MC: exp(dt_scan w) */
  double vx, vy, wz;     /* MC: the body velocity [m/s, m/s, rad/s]; 0 in rigid mode */
  int32_t inliers;       /* of the winning hypothesis (the refit runs over them) */
  int32_t hypotheses;    /* evaluated: h_stop + 1 */
  int32_t gn_iterations; /* MC: Gauss-Newton steps of the refit */
  int32_t status;        /* 0 ok; 1 fewer than 2 matches; 2 more than 16384 matches; 4 no hypothesis had 2 inliers (1, 2, 4: identity) */
} rsx_ransac_result;

int rsx_ransac_default_params(rsx_ransac_params *p);
int rsx_ransac_create(int device, rsx_ransac **out);
int rsx_ransac_destroy(rsx_ransac *h);
/* n_pairs scan pairs laid out as for rsx_orora_register_batch (offsets checked likewise); dt [matches] (NULL unless RSX_RANSAC_MOTION_COMPENSATED);
 * out [n_pairs]; out_inlier (optional) [matches]: 1 for the winner's inliers.  Host buffers, synchronous. */
int rsx_ransac_estimate_batch(rsx_ransac *h, const float *src_xy, const float *dst_xy, const float *dt, const int64_t *offsets,
                              int32_t n_pairs, const rsx_ransac_params *params, rsx_ransac_result *out, uint8_t *out_inlier);
/* device buffers, asynchronous on `stream`; never allocates or synchronises; d_offsets are trusted */
int rsx_ransac_estimate_batch_device(rsx_ransac *h, const float *d_src_xy, const float *d_dst_xy, const float *d_dt,
                                     const int64_t *d_offsets, int32_t n_pairs, const rsx_ransac_params *params,
                                     rsx_ransac_result *d_out, uint8_t *d_out_inlier, void *stream);

/* ============================== motion and Doppler compensation of keypoints ============
 * The deskewing and Doppler switches of the upstream odometry (ORORA's options, yeti_radar_odometry's --doppler
 * configuration).  Their sources are absent from the reference checkout (empty submodule), so these entries follow the model
 * below as restated in tests/mocomp_np.py, which is the arithmetic contract -- parity unpinned.
 *   Time    the keypoint on azimuth row a was measured tau = (a + 0.5) / rows * dt_scan after its scan's start; scans
 *           start dt_scan apart (the model of rsx_odometry_set_estimator).
 *   Doppler (RSX_MOCOMP_DOPPLER, applied first) the measured range r = |p| becomes r + beta (vx x / r + vy y / r) at
 *           the measured bearing; a point with r = 0 stays.  beta [s] is signed; 0.049 is the value recalled from yeti for
 *           the Navtech CIR204-H.  Neither the value nor the SIGN CONVENTION could be checked against hardware or against
 *           upstream here: a sensor whose ranges shorten while it approaches a target has beta > 0 in this convention.
 *   Deskew  (RSX_MOCOMP_DESKEW) the sensor moves at a constant body velocity w = (vx, vy, wz); the point measured at tau
 *           is expressed in the sensor frame at the scan's start: p0 = exp(tau w) p = R(th) p + V(th) (vx, vy) tau,
 *           th = wz tau, V = [[A, -B], [B, A]], A = sin th / th, B = (1 - cos th) / th (the convention of rsx_ransac:
 *           dst = exp(dt w) src).
 * sin, cos, A and B are fixed polynomials in th (csrc/mocomp.hip proves their truncation error below 2^-53 relative for
 * |th| <= 0.5), evaluated in fp64 in a fixed order without fused multiply-adds; no transcendental function is called, so
 * the fp32 outputs are reproducible bit for bit.  A point with |th| > 0.5 (or a th that is not finite) is left as measured
 * -- no Doppler correction either -- and sets RSX_MOCOMP_STATUS_ANGLE in its scan's / pair's status word.
 * A handle owns a stream and the staging of the host-buffer entries; the device entries never allocate or synchronise. */

typedef struct rsx_mocomp rsx_mocomp;

typedef struct {
  double dt_scan;   /* duration of one revolution [s] (0.25: a Navtech head at 4 Hz); positive */
  double beta;      /* Doppler range shift per unit of radial velocity [s] (0.049); signed, finite */
  int32_t rows;     /* azimuth rows per scan (400); positive */
  int32_t flags;    /* RSX_MOCOMP_DESKEW | RSX_MOCOMP_DOPPLER: at least one, nothing else */
  int32_t reserved[2]; /* 0 */
} rsx_mocomp_params;
#define RSX_MOCOMP_DESKEW 1
#define RSX_MOCOMP_DOPPLER 2
#define RSX_MOCOMP_STATUS_ANGLE 1 /* status word: some point had |wz tau| > 0.5, or (matches) the pair's pose has |yaw| > 0.5 or is
                                     not finite: those points / that pair were left as measured */

int rsx_mocomp_default_params(rsx_mocomp_params *p);
int rsx_mocomp_create(int device, rsx_mocomp **out);
int rsx_mocomp_destroy(rsx_mocomp *h);
/* n_scans clouds in the offsets layout of rsx_orora_register_batch (checked likewise): scan i owns points [offsets[i], offsets[i+1]) of xy
 * (float x, y per point) and of rows (the azimuth row of each point); w [n_scans][3] doubles: (vx, vy, wz) of each scan.
 * out_xy: the compensated points, laid out like xy, a buffer of its own; out_status [n_scans] (optional): 0 or
 * RSX_MOCOMP_STATUS_ANGLE.  params = NULL: rsx_mocomp_default_params (both corrections).  Host buffers, synchronous. */
int rsx_mocomp_points_batch(rsx_mocomp *h, const float *xy, const int32_t *rows, const int64_t *offsets, int32_t n_scans, const double *w,
                            const rsx_mocomp_params *params, float *out_xy, int32_t *out_status);
/* device buffers, asynchronous on `stream`; never allocates or synchronises; d_offsets are trusted */
int rsx_mocomp_points_batch_device(rsx_mocomp *h, const float *d_xy, const int32_t *d_rows, const int64_t *d_offsets, int32_t n_scans,
                                   const double *d_w, const rsx_mocomp_params *params, float *d_out_xy, int32_t *d_out_status, void *stream);
/* The matches of n_pairs scan pairs as staged for rsx_orora_register_batch (src = the later scan's points, dst = the earlier
 * scan's), a_cur / a_prev: the azimuth rows of src / dst, pose [n_pairs][3] doubles: (x, y, yaw) of each pair in the
 * rsx_orora_result convention (dst = R(yaw) src + (x, y)).  The kernel derives the pair's velocity w = log(pose) / dt_scan
 * (the polynomials again and one division; |yaw| <= 0.5) and writes both sides compensated with it, each into the start frame
 * of its own scan: out_src = exp(tau_cur w) src, out_dst = exp(tau_prev w) dst, so that out_dst = exp(dt_scan w) out_src for a
 * static point.  out_status [n_pairs] (optional).  Host buffers, synchronous; offsets checked as above.  The device entry
 * trusts d_offsets. */
int rsx_mocomp_matches_batch(rsx_mocomp *h, const float *src_xy, const float *dst_xy, const int32_t *a_cur, const int32_t *a_prev,
                             const int64_t *offsets, int32_t n_pairs, const double *pose, const rsx_mocomp_params *params, float *out_src_xy,
                             float *out_dst_xy, int32_t *out_status);
int rsx_mocomp_matches_batch_device(rsx_mocomp *h, const float *d_src_xy, const float *d_dst_xy, const int32_t *d_a_cur, const int32_t *d_a_prev,
                                    const int64_t *d_offsets, int32_t n_pairs, const double *d_pose, const rsx_mocomp_params *params,
                                    float *d_out_src_xy, float *d_out_dst_xy, int32_t *d_out_status, void *stream);

/* ============================== cen2019 keypoint extraction ============================
 * Replaces the feature-extraction stage of the upstream file-based `odometry.cpp` entry
 * (reference README.md:27,29).  Source absent from the reference checkout (empty submodule):
 * follows the published method (oracle/cen2019_ref.c) -- parity unpinned. */

typedef struct rsx_cen2019 rsx_cen2019;

typedef struct {
  int32_t max_points; /* budget of marked regions (10000) */
  int32_t min_range;  /* first range bin considered for keypoints (58) */
} rsx_cen2019_params;

int rsx_cen2019_default_params(rsx_cen2019_params *p);
/* one handle per image shape: rows azimuths x cols range bins (MulRan/Navtech: 400 x 3360) */
int rsx_cen2019_create(int device, int32_t rows, int32_t cols, rsx_cen2019 **out);
int rsx_cen2019_destroy(rsx_cen2019 *h);
/* img: rows x row_stride bytes (host), power samples at [col_offset, col_offset+cols) of each row
 * (col_offset = 11 for MulRan polar_oxford_form rows).  out_targets: (azimuth idx, range idx) int32
 * pairs in row-major order.  If azimuths (rows floats, rad) is given, out_xy (optional) receives
 * x = (r+0.5)*resolution*cos(az), y = ...*sin(az) -- the /orora/cloud_local points.
 * *out_count = keypoints found (only the first max_targets are written). */
int rsx_cen2019_extract(rsx_cen2019 *h, const uint8_t *img, int32_t row_stride, int32_t col_offset,
                        const rsx_cen2019_params *params, const float *azimuths, float resolution,
                        int32_t *out_targets, float *out_xy, int32_t max_targets, int32_t *out_count);
/* The same for n_images scans in ONE chain of launches (a file-based sequence is known in advance: README.md:27,54-60).
 * Images image_stride_bytes apart; azimuths: rows floats shared by all images, or n_images x rows when
 * azimuths_per_image != 0.  out_targets [n_images][max_targets][2], out_xy [n_images][max_targets][2] (optional),
 * out_counts [n_images].  Host buffers, synchronous. */
int rsx_cen2019_extract_batch(rsx_cen2019 *h, const uint8_t *imgs, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride,
                              int32_t col_offset, const rsx_cen2019_params *params, const float *azimuths, int32_t azimuths_per_image,
                              float resolution, int32_t *out_targets, float *out_xy, int32_t max_targets, int32_t *out_counts);
/* Device buffers in and out, asynchronous on `stream`, no host synchronisation anywhere in the chain: d_targets / d_xy /
 * d_counts as above in HBM (d_xy, d_counts optional), ready for rsx_frontend_describe_device without a host hop. */
int rsx_cen2019_extract_batch_device(rsx_cen2019 *h, const uint8_t *d_imgs, int32_t n_images, int64_t image_stride_bytes,
                                     int32_t row_stride, int32_t col_offset, const rsx_cen2019_params *params, const float *d_azimuths,
                                     int32_t azimuths_per_image, float resolution, int32_t *d_targets, float *d_xy, int32_t max_targets,
                                     int32_t *d_counts, void *stream);

/* ============================== cen2018 keypoint extraction ============================
 * The other keypoint extractor of the upstream file-based `odometry.cpp` entry (yeti_radar_odometry's
 * keypoint_extraction = 0, Cen & Newman ICRA 2018).  Source absent from the reference checkout (empty submodule): follows
 * the method as restated in tests/cen2018_np.py -- parity unpinned.  Per azimuth row: q = fft - mean(fft), p = q smoothed
 * along range by a 1 x (3 sigma_gauss) Gaussian (reflect 101), sigma = the noise level of the negative q, and one keypoint
 * at the median bin of every run of consecutive range bins >= min_range with y = q (1 - nqp) + p (nqp - npp) > zq * sigma.
 * Same argument shapes, output layout (row-major (azimuth idx, range idx), x = (r+0.5)*resolution*cos(az), ...) and
 * truncation rules as the cen2019 group above; *out_count / out_counts report every keypoint found.
 * Invalid parameters (an even or non-positive sigma_gauss or one above 85, a negative min_range, a zq that is not finite)
 * return RSX_ERR_BAD_ARG.  Device workspace per handle: rows x (cols / 2 + 1) x 2 bytes of per-row keypoints + rows x 4
 * bytes of counts per image of a sub-batch (<= 128 images: 172 MB for 400 x 3360 scans), plus the host entries' staging
 * (images, keypoints, points of one sub-batch). */

typedef struct rsx_cen2018 rsx_cen2018;

typedef struct {
  float zq;            /* threshold in noise sigmas (3.0) */
  int32_t sigma_gauss; /* Gaussian sigma in range bins, odd, 1 .. 85; the filter has 3 sigma_gauss taps (17) */
  int32_t min_range;   /* first range bin considered for keypoints (58) */
  int32_t reserved;    /* 0 */
} rsx_cen2018_params;

int rsx_cen2018_default_params(rsx_cen2018_params *p);
/* one handle per image shape: rows (1 .. 4096) azimuths x cols (1 .. 8192) range bins */
int rsx_cen2018_create(int device, int32_t rows, int32_t cols, rsx_cen2018 **out);
int rsx_cen2018_destroy(rsx_cen2018 *h);
int rsx_cen2018_extract(rsx_cen2018 *h, const uint8_t *img, int32_t row_stride, int32_t col_offset,
                        const rsx_cen2018_params *params, const float *azimuths, float resolution,
                        int32_t *out_targets, float *out_xy, int32_t max_targets, int32_t *out_count);
int rsx_cen2018_extract_batch(rsx_cen2018 *h, const uint8_t *imgs, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride,
                              int32_t col_offset, const rsx_cen2018_params *params, const float *azimuths, int32_t azimuths_per_image,
                              float resolution, int32_t *out_targets, float *out_xy, int32_t max_targets, int32_t *out_counts);
/* two launches per 128 images, no host synchronisation */
int rsx_cen2018_extract_batch_device(rsx_cen2018 *h, const uint8_t *d_imgs, int32_t n_images, int64_t image_stride_bytes,
                                     int32_t row_stride, int32_t col_offset, const rsx_cen2018_params *params, const float *d_azimuths,
                                     int32_t azimuths_per_image, float resolution, int32_t *d_targets, float *d_xy, int32_t max_targets,
                                     int32_t *d_counts, void *stream);

/* ============================== k-strongest keypoint extraction ========================
 * The detector of CFEAR radar odometry (Adolfsson et al.: k = 12, z_min = 60) with a separation rule: on every azimuth the
 * k strongest returns above a fixed power floor.  No noise model, one read of the image, and a hard budget of rows x k
 * keypoints per scan.  Not part of the reference; the rule below is restated in tests/kstrongest_np.py, which is the
 * arithmetic contract.  Integers only: the keypoints equal the restatement's bit for bit.
 * Per azimuth row, v[j] = the power byte of range bin j, 0 <= j < cols, s = min_separation:
 *   1. key[j] = (v[j] << 16) | (0xFFFF - j): unique within a row; a higher key is stronger, on equal power the nearer bin wins
 *   2. win[j] = max key[i] over max(0, j - s) <= i <= min(cols - 1, j + s): the window is cut at the row's ends (it never sees
 *      metadata bytes, row padding or another row) and runs over raw power whatever z_min / min_range say
 *   3. bin j is a candidate iff key[j] == win[j], v[j] >= z_min and min_range <= j < hi, hi = cols when max_range == 0, else
 *      min(max_range, cols)
 *   4. the row's keypoints are the min(k, #candidates) candidates of highest key, written in ascending j
 *   5. the image's keypoints are the rows' keypoints in row-major order
 * So s = 0 is CFEAR's plain rule, and with s > 0 any two keypoints of a row are more than s bins apart.
 * Why the default is s = 5: the plain rule picks runs of adjacent range bins on a strong reflector.  In the odometry
 * pipeline a Cartesian pixel is 0.2592 m and a range bin 0.0595 m, so adjacent bins get identical ORB-style descriptors and
 * the ratio test of knnMatch drops them all.  Measured on the CPU (restatement -> oracle front end -> cross-checked ratio
 * matches -> max-clique selection -> ORORA; synth.polar_sequence(11, 5), k = 12, z_min = 60; 4800 keypoints per scan with
 * every rule; every pair status 0):
 *     min_separation   cross-checked matches per pair   worst pair error
 *     0 (plain rule)   59 - 73                          0.056 m / 4.1e-3 rad
 *     1                525 - 715                        0.046 m / 4.2e-3 rad
 *     5                550 - 722                        0.045 m / 3.9e-3 rad
 * Same argument shapes, output layout ((azimuth idx, range idx) int32 pairs, x = (r+0.5)*resolution*cos(az), ...) and
 * truncation rules as the cen2019 group above; *out_count / out_counts report every keypoint found, only the first
 * max_targets are written.  Parameters out of range return RSX_ERR_BAD_ARG.  Device workspace per handle: rows x k x 2 bytes
 * of per-row keypoints + rows x 4 bytes of counts per image of a sub-batch (<= 128 images: 1.4 MB for 400 x 3360 scans at
 * k = 12), plus the host entries' staging (images, keypoints, points of one sub-batch). */

typedef struct rsx_kstrongest rsx_kstrongest;

typedef struct {
  int32_t k;              /* keypoints per azimuth at most, 1 .. 128 (12) */
  int32_t z_min;          /* power floor, 0 .. 255 (60) */
  int32_t min_range;      /* first range bin considered for keypoints, >= 0 (58) */
  int32_t max_range;      /* one past the last range bin considered, >= 0; 0 = cols (0) */
  int32_t min_separation; /* s, 0 .. 32; 0 = CFEAR's plain rule (5) */
  int32_t reserved;       /* 0 */
} rsx_kstrongest_params;

int rsx_kstrongest_default_params(rsx_kstrongest_params *p);
/* one handle per image shape: rows (1 .. 4096) azimuths x cols (1 .. 8192) range bins */
int rsx_kstrongest_create(int device, int32_t rows, int32_t cols, rsx_kstrongest **out);
int rsx_kstrongest_destroy(rsx_kstrongest *h);
int rsx_kstrongest_extract(rsx_kstrongest *h, const uint8_t *img, int32_t row_stride, int32_t col_offset,
                           const rsx_kstrongest_params *params, const float *azimuths, float resolution,
                           int32_t *out_targets, float *out_xy, int32_t max_targets, int32_t *out_count);
int rsx_kstrongest_extract_batch(rsx_kstrongest *h, const uint8_t *imgs, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride,
                                 int32_t col_offset, const rsx_kstrongest_params *params, const float *azimuths, int32_t azimuths_per_image,
                                 float resolution, int32_t *out_targets, float *out_xy, int32_t max_targets, int32_t *out_counts);
/* two launches per 128 images, no host synchronisation.  Only bytes inside each image's rows x row_stride bytes are read,
 * whatever the alignment of d_imgs. */
int rsx_kstrongest_extract_batch_device(rsx_kstrongest *h, const uint8_t *d_imgs, int32_t n_images, int64_t image_stride_bytes,
                                        int32_t row_stride, int32_t col_offset, const rsx_kstrongest_params *params, const float *d_azimuths,
                                        int32_t azimuths_per_image, float resolution, int32_t *d_targets, float *d_xy, int32_t max_targets,
                                        int32_t *d_counts, void *stream);

/* ============================== CA-CFAR / BFAR keypoint extraction =====================
 * A constant false-alarm rate detector: a range bin is compared with the noise AROUND it, not with a row-wide statistic or a
 * fixed floor.  The threshold is affine in the local noise estimate Z (the mean of the training cells), T = a Z + b -- BFAR,
 * the detector CFEAR's authors replaced the fixed floor with (Alhashimi, Adolfsson et al.).  b = 0 is cell-averaging CFAR,
 * a = 0 is the fixed floor of k-strongest; greatest-of and smallest-of the two sides are the standard variants for clutter
 * edges and for neighbouring targets.  On each azimuth the k strongest detections are kept, under k-strongest's separation
 * rule.  Not part of the reference; the rule below is restated in tests/cfar_np.py, which is the arithmetic contract.
 * Integers only: the keypoints equal the restatement's bit for bit.
 * Per azimuth row, v[j] = the power byte of range bin j, 0 <= j < cols; t = train, g = guard, A = scale_q8 (a = A / 256),
 * B = offset, s = min_separation:
 *   1. key[j] and win[j] exactly as in k-strongest steps 1 and 2: raw power, the window cut at the row's ends
 *   2. training cells of bin j: left, the bins i with j - g - t <= i <= j - g - 1 and i >= 0; right, the bins i with
 *      j + g + 1 <= i <= j + g + t and i <= cols - 1.  Their sums and counts are S_L, n_L, S_R, n_R.  The cells are cut at the
 *      row's ends (they never see metadata bytes, row padding or another row) and run over raw power whatever min_range and
 *      max_range say
 *   3. noise (S, n) by mode: RSX_CFAR_CA (0, cell averaging) (S_L + S_R, n_L + n_R); RSX_CFAR_GO (1, greatest-of) the side
 *      with the larger mean -- left iff S_L n_R >= S_R n_L; RSX_CFAR_SO (2, smallest-of) the side with the smaller mean.  In
 *      modes 1 and 2 an empty side (n = 0) gives way to the other; on equal means either side gives the same verdict in step 4
 *   4. detection: 256 n v[j] > A S + 256 B n when n > 0; v[j] > B when n = 0 (a row too short to have any training cell).
 *      Strict, so a flat row at A = 256 detects nothing.  Within the limits below both sides stay below 2^31: the right side
 *      is at most 65535 x 32640 + 256 x 255 x 128 = 2 147 418 240
 *   5. bin j is a candidate iff key[j] == win[j], it is a detection, and min_range <= j < hi (hi as in k-strongest)
 *   6. steps 4 and 5 of k-strongest: the min(k, #candidates) candidates of highest key in ascending j, rows in row-major order
 * So A = 0 is k-strongest with z_min = B + 1, and B = 0 is plain CA-CFAR with a = A / 256.
 * The defaults of scale_q8 and offset come from the study that chose k-strongest's min_separation, on the CPU (restatement ->
 * oracle front end -> cross-checked ratio matches -> max-clique selection -> ORORA; synth.polar_sequence(11, 5); k = 12,
 * train = 20, guard = 2, mode 0, min_separation = 5; tools/cfar_defaults_study.py): the setting with the smallest worst pair
 * error among those whose every pair has status 0.
 * Translation error decides, the yaw error breaks ties at the millimetre; every pair of every row has status 0:
 *     setting                    keypoints per scan   cross-checked matches per pair   worst pair error
 *     k-strongest, z_min = 60    4800                 550 - 722                        0.045 m / 3.9e-3 rad
 *     A =  512, B =  0           4800                 512 - 681                        0.036 m / 3.8e-3 rad
 *     A =  512, B = 20           4800                 497 - 666                        0.023 m / 3.3e-3 rad
 *     A =  512, B = 40           4800                 472 - 651                        0.025 m / 3.6e-3 rad
 *     A =  768, B =  0           4800                 454 - 592                        0.024 m / 2.8e-3 rad
 *     A =  768, B = 20           4799 - 4800          413 - 560                        0.021 m / 3.4e-3 rad   <- the defaults
 *     A =  768, B = 40           4405 - 4488          353 - 470                        0.021 m / 4.4e-3 rad
 *     A = 1024, B =  0           4665 - 4707          301 - 383                        0.026 m / 3.8e-3 rad
 *     A = 1024, B = 20           3049 - 3152          200 - 266                        0.028 m / 4.6e-3 rad
 *     A = 1024, B = 40           1679 - 1792          123 - 160                        0.031 m / 4.9e-3 rad
 *     A = 1536, B =  0           713 - 772            45 - 60                          0.103 m / 5.4e-3 rad
 *     A = 1536, B = 20           379 - 406            15 - 30                          0.106 m / 3.1e-3 rad
 *     A = 1536, B = 40           191 - 218            8 - 16                           0.166 m / 3.3e-3 rad
 * A synthetic sequence only: on it the detector halves k-strongest's worst pair error with fewer matches; no real radar
 * data has been through it.
 * Same argument shapes, output layout, truncation rules and create limits as the k-strongest group above.  Parameters outside
 * the limits in the struct below return RSX_ERR_BAD_ARG.  Device workspace per handle: as k-strongest's. */

#define RSX_CFAR_CA 0 /* cell averaging: both sides */
#define RSX_CFAR_GO 1 /* greatest-of: the side with the larger mean */
#define RSX_CFAR_SO 2 /* smallest-of: the side with the smaller mean */

typedef struct rsx_cfar rsx_cfar;

typedef struct {
  int32_t k;              /* keypoints per azimuth at most, 1 .. 128 (12) */
  int32_t train;          /* t, training cells on each side, 1 .. 64 (20) */
  int32_t guard;          /* g, guard cells on each side between the bin and its training cells, 0 .. 16 (2) */
  int32_t scale_q8;       /* A = 256 a, 0 .. 65535 (768: a = 3) */
  int32_t offset;         /* B, 0 .. 255 (20) */
  int32_t mode;           /* RSX_CFAR_CA / _GO / _SO (RSX_CFAR_CA) */
  int32_t min_range;      /* first range bin considered for keypoints, >= 0 (58) */
  int32_t max_range;      /* one past the last range bin considered, >= 0; 0 = cols (0) */
  int32_t min_separation; /* s, 0 .. 32 (5) */
  int32_t reserved;       /* 0 */
} rsx_cfar_params;

int rsx_cfar_default_params(rsx_cfar_params *p);
/* one handle per image shape: rows (1 .. 4096) azimuths x cols (1 .. 8192) range bins */
int rsx_cfar_create(int device, int32_t rows, int32_t cols, rsx_cfar **out);
int rsx_cfar_destroy(rsx_cfar *h);
int rsx_cfar_extract(rsx_cfar *h, const uint8_t *img, int32_t row_stride, int32_t col_offset, const rsx_cfar_params *params,
                     const float *azimuths, float resolution, int32_t *out_targets, float *out_xy, int32_t max_targets, int32_t *out_count);
int rsx_cfar_extract_batch(rsx_cfar *h, const uint8_t *imgs, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride, int32_t col_offset,
                           const rsx_cfar_params *params, const float *azimuths, int32_t azimuths_per_image, float resolution,
                           int32_t *out_targets, float *out_xy, int32_t max_targets, int32_t *out_counts);
/* two launches per 128 images, no host synchronisation.  Only bytes inside each image's rows x row_stride bytes are read,
 * whatever the alignment of d_imgs. */
int rsx_cfar_extract_batch_device(rsx_cfar *h, const uint8_t *d_imgs, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride,
                                  int32_t col_offset, const rsx_cfar_params *params, const float *d_azimuths, int32_t azimuths_per_image,
                                  float resolution, int32_t *d_targets, float *d_xy, int32_t max_targets, int32_t *d_counts, void *stream);

/* ============================== CFEAR surface points and registration ==================
 * What the k-strongest detector feeds in CFEAR radar odometry (Adolfsson et al.): no descriptors and no matcher.  The
 * filtered returns of a scan are summarised as ORIENTED SURFACE POINTS -- the mean and the surface normal of the returns
 * within a radius -- and two scans are registered by minimising a robust POINT-TO-LINE cost between their surface points.
 * CFEAR's own code is not part of the reference checkout: the rules below are restated in tests/cfear_np.py, which is the
 * arithmetic contract -- parity unpinned.
 * Surface points of one cloud (n <= RSX_CFEAR_MAX_POINTS points, float x, y, sensor frame), r = radius, all in fp64:
 *   - cell of a point: ix = floor(x / r), iy = floor(y / r); a point with ix or iy outside [-64, 64) (non-finite included) is
 *     ignored and sets RSX_CFEAR_STATUS_RANGE (+-224 m at r = 3.5)
 *   - per occupied cell, in ascending (iy, ix): c = the mean of the cell's own points; the neighbours are the points p of
 *     the 3 x 3 block of cells with |p - c|^2 <= r^2 (dy outer, dx inner, input order inside a cell); fewer than min_points:
 *     no surface point; mu = their mean, S = their sample covariance (divided by m - 1); lambda_max/min = h +- sqrt(((sxx -
 *     syy) / 2)^2 + sxy^2), h = (sxx + syy) / 2; kept iff lambda_min > 0 and lambda_max <= max_condition x lambda_min; the
 *     normal is the unit eigenvector of lambda_min (from the row of S - lambda_min I with the larger pivot), turned to face
 *     the sensor (n.mu <= 0)
 *   - every sum runs sequentially in the order above, nothing is fused: the records equal the restatement's bit for bit.
 *     Two cells that see the same neighbour set give the same record but for `cell`; both are kept
 * Registration of a pair (src = the later scan's records, dst = the earlier scan's; dst = R(yaw) src + (x, y), as for
 * rsx_orora_result), Gauss-Newton from the start pose, per iteration: q = R mu_i + t, m = R n_i; the correspondence of src
 * record i is the dst record j of smallest |q - mu_j|^2 among those with |q - mu_j|^2 <= radius^2 and m.n_j >=
 * cos_max_normal_angle (lowest j on a tie; none is allowed); residual e = n_j.(q - mu_j), Huber weight 1 for |e| <=
 * huber_delta else huber_delta / |e|; the 3 x 3 normal equations are solved by LDL^T without pivoting in the order (x, y,
 * yaw); the loop ends when the step's norm is < step_epsilon, or at max_iterations.  A pair's result does not depend on its
 * place in the batch; no host round trip inside the loop.
 * The objective: that is CFEAR's point-to-line cost with the Huber loss and no weights, the default.  rsx_cfear_params.cost, loss
 * and weights choose among the family CFEAR publishes, in every entry that takes the struct (pairs, keyframes, the tracker pushes,
 * rsx_odometry_set_cfear); the rules are restated in tests/cfear_cost_np.py (the arithmetic contract; parity unpinned).  The
 * correspondence rule stays as above.  For a correspondence (src record i, dst record j of a keyframe k; a pair is one keyframe at
 * the identity): d = q - mu_j, m = the src normal in the keyframe's frame, t_j = (-n_jy, n_jx), p' = R'(yaw_r) mu_i (the derivative
 * of R(yaw_r) mu_i in yaw_r).  A residual row along a direction u with scale s has e = s (u.d) and J = (s R(yaw_k) u, s (u.p')).
 *   cost    RSX_CFEAR_COST_P2L: one row (n_j, 1).  RSX_CFEAR_COST_P2P: two rows, (n_j, 1) then (t_j, 1): the whole of d.
 *           RSX_CFEAR_COST_P2D: two rows, (n_j, 1 / sqrt(lambda_min_j)) then (t_j, 1 / sqrt(lambda_max_j)): the Mahalanobis distance of
 *           q under the dst record's distribution.  A record is VALID when lambda_min > 0, lambda_max >= lambda_min and both are
 *           finite; under P2D a correspondence whose dst record is not valid is skipped and not counted
 *   loss    on s2 = the sum of the rows' e^2, a = sqrt(s2) (one row: |e|), delta = huber_delta -- under P2D a dimensionless threshold
 *           on the Mahalanobis distance, not metres.  RSX_CFEAR_LOSS_HUBER: w = 1 if a <= delta else delta / a, rho = s2 / 2 inside,
 *           delta (a - delta / 2) outside.  RSX_CFEAR_LOSS_CAUCHY: w = 1 / (1 + s2 / delta^2), rho = (delta^2 / 2) log(1 + s2 / delta^2).
 *           RSX_CFEAR_LOSS_NONE: w = 1, rho = s2 / 2
 *   weights 0: v = 1.  1: v = w_dir w_plan w_num, how well the two surface points resemble each other: w_dir = max(m.n_j, 0); w_plan =
 *           2 min(p_i, p_j) / (p_i + p_j) with p = log(1 + lambda_max / lambda_min) of a record; w_num = 2 min(N_i, N_j) / (N_i + N_j)
 *           with N = n_points.  With weights a correspondence whose src or dst record is not valid is skipped and not counted
 * H += v w J J^T and g += v w J e over the rows (n first, then t), cost += v rho, correspondences += 1.  The solve, the pivot and step
 * tests and the statuses are the same for every objective.  A wall whose records share one normal is status 5 under P2L (nothing
 * constrains motion along it) and registers under P2P and P2D. */

typedef struct rsx_cfear rsx_cfear;

#define RSX_CFEAR_COST_P2L 0    /* rsx_cfear_params.cost: point-to-line */
#define RSX_CFEAR_COST_P2P 1    /* point-to-point */
#define RSX_CFEAR_COST_P2D 2    /* point-to-distribution */
#define RSX_CFEAR_LOSS_HUBER 0  /* rsx_cfear_params.loss */
#define RSX_CFEAR_LOSS_CAUCHY 1
#define RSX_CFEAR_LOSS_NONE 2   /* least squares */

#define RSX_CFEAR_MAX_POINTS 16384        /* points of one scan */
#define RSX_CFEAR_MAX_SURFACE_POINTS 4096 /* records written per scan, and records of one side of a registered pair */
#define RSX_CFEAR_STATUS_RANGE 1          /* scan status word: some point lay outside the 128 x 128 cell grid (or was not finite) */
#define RSX_CFEAR_STATUS_POINTS 2         /* scan status word (device entry only): more than RSX_CFEAR_MAX_POINTS points, no record
                                             (the host entry refuses such a scan with RSX_ERR_BAD_ARG) */

typedef struct {
  double radius;               /* r: cell side, neighbourhood radius and correspondence radius [m], > 0 (3.5) */
  double max_condition;        /* lambda_max / lambda_min at most, >= 1 (1e5) */
  double cos_max_normal_angle; /* correspondences need m.n_j >= this, in [-1, 1] (cos 30 deg) */
  double huber_delta;          /* delta of the loss, Huber's or Cauchy's, > 0 (0.1): [m], under RSX_CFEAR_COST_P2D dimensionless */
  double step_epsilon;         /* the loop ends when |step| < this, >= 0 (1e-6) */
  int32_t min_points;          /* neighbours a surface point needs, >= 2 (6) */
  int32_t max_iterations;      /* 1 .. 200 (50) */
  int32_t min_correspondences; /* >= 1 (6) */
  int32_t cost;                /* RSX_CFEAR_COST_* (RSX_CFEAR_COST_P2L) */
  int32_t loss;                /* RSX_CFEAR_LOSS_* (RSX_CFEAR_LOSS_HUBER) */
  int32_t weights;             /* 1: weigh every correspondence by the resemblance of its surface points; 0: no (0) */
} rsx_cfear_params;

typedef struct {
  float x, y;                   /* mean of the neighbours */
  float nx, ny;                 /* unit normal, facing the sensor */
  float lambda_max, lambda_min; /* eigenvalues of the sample covariance */
  int32_t n_points;             /* neighbours */
  int32_t cell;                 /* (iy + 64) * 128 + (ix + 64) */
} rsx_cfear_surface_point;      /* 32 bytes */

typedef struct {
  double x, y, yaw;        /* dst = R(yaw) src + (x, y) */
  double cost;             /* the loss (Huber's by default) summed over the last linearisation made */
  int32_t iterations;      /* steps taken */
  int32_t correspondences; /* of the last linearisation made */
  int32_t status;          /* 0 ok; 1 a side has no surface points; 2 a side has more than RSX_CFEAR_MAX_SURFACE_POINTS; 4 fewer than
                              min_correspondences; 5 degenerate normal equations (a pivot not > 1e-12 x its diagonal entry); 8
                              max_iterations reached (the pose is still returned).  1, 2: the start pose; 4, 5: the pose reached so far */
  int32_t reserved;
} rsx_cfear_result;

int rsx_cfear_default_params(rsx_cfear_params *p);
int rsx_cfear_create(int device, rsx_cfear **out);
int rsx_cfear_destroy(rsx_cfear *h);
/* n_scans clouds; scan i owns points [offsets[i], offsets[i + 1]) of xy (float x, y per point); offsets as for
 * rsx_orora_register_batch (checked), and no scan may hold more than RSX_CFEAR_MAX_POINTS points.  Scan i's records go to
 * out_records + i * max_records (1 <= max_records <= RSX_CFEAR_MAX_SURFACE_POINTS); out_counts[i] reports every record found,
 * only the first max_records are written; out_status[i] is the scan's status word (either may be NULL).  Host buffers,
 * synchronous.  One workgroup per scan, one launch. */
int rsx_cfear_surface_points_batch(rsx_cfear *h, const float *xy, const int64_t *offsets, int32_t n_scans, const rsx_cfear_params *params,
                                   rsx_cfear_surface_point *out_records, int32_t max_records, int32_t *out_counts, int32_t *out_status);
/* device buffers, asynchronous on `stream`, no allocation; d_offsets are trusted (a scan above the cap gets
 * RSX_CFEAR_STATUS_POINTS and no record).  d_counts is required here */
int rsx_cfear_surface_points_batch_device(rsx_cfear *h, const float *d_xy, const int64_t *d_offsets, int32_t n_scans,
                                          const rsx_cfear_params *params, rsx_cfear_surface_point *d_records, int32_t max_records,
                                          int32_t *d_counts, int32_t *d_status, void *stream);
/* n_pairs pairs; pair i registers src records [src_offsets[i], src_offsets[i + 1]) to dst records [dst_offsets[i],
 * dst_offsets[i + 1]); init: [n_pairs][3] doubles x, y, yaw, NULL = identity.  Host buffers, synchronous.  One launch: the joint
 * registration below with dst i as the one keyframe of job i at the identity pose, through the cell index. */
int rsx_cfear_register_batch(rsx_cfear *h, const rsx_cfear_surface_point *src, const int64_t *src_offsets,
                             const rsx_cfear_surface_point *dst, const int64_t *dst_offsets, int32_t n_pairs, const double *init,
                             const rsx_cfear_params *params, rsx_cfear_result *out);
/* device buffers (d_init too, or NULL), asynchronous on `stream`; the offsets are trusted.  The handle's index workspace grows
 * with min(n_pairs, 256); no allocation otherwise */
int rsx_cfear_register_batch_device(rsx_cfear *h, const rsx_cfear_surface_point *d_src, const int64_t *d_src_offsets,
                                    const rsx_cfear_surface_point *d_dst, const int64_t *d_dst_offsets, int32_t n_pairs,
                                    const double *d_init, const rsx_cfear_params *params, rsx_cfear_result *d_out, void *stream);

/* ---- CFEAR scan-to-keyframes registration and the keyframe tracker (csrc/cfear_track.hip) ----
 * CFEAR registers a scan JOINTLY against the last few keyframes, from a constant-velocity prediction, and makes a new keyframe
 * only after enough motion.  The rules are restated in tests/cfear_track_np.py (the arithmetic contract; parity unpinned).
 * Poses are (x, y, yaw) with map = R(yaw) p + (x, y); A o B = (A.x + (c B.x - s B.y), A.y + (s B.x + c B.y), A.yaw + B.yaw) and
 * A^-1 o B = (c dx + s dy, c dy - s dx, B.yaw - A.yaw) with c, s = cos, sin(A.yaw), (dx, dy) = B's position - A's; no yaw is wrapped.
 * Joint registration: K keyframes (1 .. RSX_CFEAR_MAX_KEYFRAMES), each with records and a pose P_k in the map frame; the result
 * is the scan's pose in the map frame.  Per iteration and keyframe the scan's pose is taken in the keyframe's frame (yaw_r = yaw -
 * yaw_k, t_r = R(-yaw_k)((x, y) - (x_k, y_k))), correspondence, residual and weight are the pair rule's above, J = (R(yaw_k) n_j,
 * n_j.(R'(yaw_r) mu_i)); H, g, cost and the correspondence count are summed over every (record, keyframe); then the pair rule's
 * solve, step test and statuses.  Status 1: the src or every keyframe is empty (an empty keyframe among others is skipped); 2: a
 * side above RSX_CFEAR_MAX_SURFACE_POINTS.  With K = 1 and P_1 = (0, 0, 0) the result equals rsx_cfear_register_batch's byte for
 * byte.  The correspondence search goes through a 128 x 128 cell index of each keyframe (cell side = radius, built once per
 * keyframe) or, search = 1, by brute force over the keyframe's records in ascending index: the same bytes either way.
 * Tracker, per sequence: state = the last pose P, the last motion M, a ring of at most n_keyframes keyframes.  Scan 0: P = 0, it is
 * the first keyframe (flag 1), its registration result is all zero.  Scan i: start = P o M (predict) or P; registered against the
 * ring.  Status 0 / 8: M = P^-1 o P_new, P = P_new, and the scan becomes a keyframe (flag 1, evicting the oldest of a full ring)
 * when its distance from the NEWEST keyframe's pose is > keyframe_distance or |remainder(yaw - yaw_kf, 2 pi)| > keyframe_rotation.
 * Status 1, 2, 4, 5: P = start, M stays, and a scan of 1 .. RSX_CFEAR_MAX_SURFACE_POINTS records becomes the ring's only entry
 * at `start` (flag 2, re-anchored). */
#define RSX_CFEAR_MAX_KEYFRAMES 4
#define RSX_CFEAR_SEARCH_CELLS 0 /* rsx_cfear_track_params.search: the keyframe's cell index */
#define RSX_CFEAR_SEARCH_BRUTE 1 /* every record of the keyframe */

typedef struct {
  double keyframe_distance; /* [m], >= 0 (1.5) */
  double keyframe_rotation; /* [rad], >= 0 (5 deg) */
  int32_t n_keyframes;      /* ring size, 1 .. RSX_CFEAR_MAX_KEYFRAMES (3) */
  int32_t predict;          /* 1: start from the constant-velocity prediction P o M; 0: from P (1) */
  int32_t search;           /* RSX_CFEAR_SEARCH_* (RSX_CFEAR_SEARCH_CELLS) */
  int32_t reserved[2];      /* 0 */
  int32_t compensate;       /* 1: motion compensation inside the tracker (below; the timed pushes only); 0: none (0) */
} rsx_cfear_track_params;

typedef struct {
  double x, y, yaw;     /* the scan's pose in the frame of the sequence's first scan */
  rsx_cfear_result reg; /* of its registration against the ring (x, y, yaw: the pose it returned in that frame); scan 0: zeros */
  int32_t keyframe;     /* 0 no; 1 the scan became a keyframe; 2 re-anchored: the ring was replaced by this scan */
  int32_t n_keyframes;  /* keyframes it was registered against */
} rsx_cfear_track_result; /* 80 bytes */

int rsx_cfear_default_track_params(rsx_cfear_track_params *p);
/* n_jobs jobs; job i registers src records [src_offsets[i], src_offsets[i + 1]) jointly to the keyframes [kf_job_offsets[i],
 * kf_job_offsets[i + 1]) (1 .. RSX_CFEAR_MAX_KEYFRAMES of them, checked); keyframe g owns records [kf_offsets[g], kf_offsets[g + 1])
 * of kf and the pose kf_poses[3 g ..]; init: [n_jobs][3] start poses in the map frame, NULL = identity.  Of `track` (NULL = the
 * defaults) only `search` acts here.  Host buffers, synchronous.  One workgroup per job, one launch. */
int rsx_cfear_register_keyframes_batch(rsx_cfear *h, const rsx_cfear_surface_point *src, const int64_t *src_offsets,
                                       const rsx_cfear_surface_point *kf, const int64_t *kf_offsets, const int64_t *kf_job_offsets,
                                       const double *kf_poses, int32_t n_jobs, const double *init, const rsx_cfear_params *params,
                                       const rsx_cfear_track_params *track, rsx_cfear_result *out);
/* device buffers, asynchronous on `stream`; the offsets are trusted: a job without a keyframe gets status 1, one with more than
 * RSX_CFEAR_MAX_KEYFRAMES status 2.  The handle's index workspace grows with min(n_jobs, 256); no allocation otherwise */
int rsx_cfear_register_keyframes_batch_device(rsx_cfear *h, const rsx_cfear_surface_point *d_src, const int64_t *d_src_offsets,
                                              const rsx_cfear_surface_point *d_kf, const int64_t *d_kf_offsets,
                                              const int64_t *d_kf_job_offsets, const double *d_kf_poses, int32_t n_jobs,
                                              const double *d_init, const rsx_cfear_params *params,
                                              const rsx_cfear_track_params *track, rsx_cfear_result *d_out, void *stream);

/* n_sequences independent sequences tracked side by side, one workgroup each, the state (pose, motion, ring with its cell
 * index) resident in HBM between calls */
typedef struct rsx_cfear_tracker rsx_cfear_tracker;
int rsx_cfear_tracker_create(int device, int32_t n_sequences, rsx_cfear_tracker **out);
int rsx_cfear_tracker_destroy(rsx_cfear_tracker *h);
/* every sequence starts again at its scan 0; the next push may carry other parameters */
int rsx_cfear_tracker_reset(rsx_cfear_tracker *h);
/* sequence q continues with its next n_scans[q] >= 0 scans; the scans lie sequence after sequence: scan j of this call's sum
 * n_scans owns records [offsets[j], offsets[j + 1]) and gets out[j].  One launch over all scans of all sequences, no host round
 * trip between scans.  Results do not depend on how a sequence is cut into pushes; params and track (NULL = defaults) must equal
 * those of the previous push since create / reset (RSX_ERR_BAD_ARG otherwise).  Host buffers, synchronous. */
int rsx_cfear_tracker_push(rsx_cfear_tracker *h, const rsx_cfear_surface_point *records, const int64_t *offsets, const int32_t *n_scans,
                           const rsx_cfear_params *params, const rsx_cfear_track_params *track, rsx_cfear_track_result *out);
/* device buffers (d_n_scans too), asynchronous on `stream`, no allocation; offsets trusted */
int rsx_cfear_tracker_push_device(rsx_cfear_tracker *h, const rsx_cfear_surface_point *d_records, const int64_t *d_offsets,
                                  const int32_t *d_n_scans, const rsx_cfear_params *params, const rsx_cfear_track_params *track,
                                  rsx_cfear_track_result *d_out, void *stream);

/* ---- CFEAR motion compensation: surface points with times, compensation of records, the two-pass tracker ----
 * A spinning radar measures a scan over one revolution; the sensor's motion during it shears the scan.  The rules are restated in
 * tests/cfear_mocomp_np.py (the arithmetic contract; parity unpinned).  Doppler on records is out of scope.
 * Time of a record: the timed surface-point entries take the azimuth row of every point (0 .. n_rows - 1, as for
 * rsx_mocomp_points_batch; 1 <= n_rows <= 65536) and give every record tau in [0, 1], the fraction of the revolution at which it
 * was measured: the CIRCULAR mean of its neighbours' rows.  With the neighbours in the order of the surface-point rule, rows
 * a_1 .. a_m, and h = n_rows / 2 (integer division): d_k = ((a_k - a_1 + h) mod n_rows, non-negative) - h, S = sum d_k (integers),
 * u = ((double)a_1 + (double)S / (double)m) + 0.5, wrapped once into [0, n_rows) (u < 0: u + n_rows; else u >= n_rows: u - n_rows),
 * tau = (float)(u / n_rows).  Neighbours on both sides of the row 0 / row n_rows - 1 seam give a time near the seam, not 0.5.
 * The records are rsx_cfear_surface_points_batch's byte for byte.
 * Compensation of a record measured at tau under `motion` = (x, y, yaw), the sensor's motion over one scan period in the
 * rsx_orora_result convention: rsx_mocomp's deskewing with dt_scan = 1 and no Doppler term.  (vx, vy, wz) = the velocity of the
 * motion (rsx_mocomp above, dt_scan = 1); th = wz tau; sn, cs, A, B = rsx_mocomp's fixed polynomials at th;
 *   x' = (cs x - sn y) + (A vx - B vy) tau,  y' = (sn x + cs y) + (B vx + A vy) tau,  n' = (cs nx - sn ny, sn nx + cs ny),
 * fp64 in this order, nothing fused, rounded to the record's floats once; every other field is copied.  A motion with not
 * |yaw| <= 0.5 or a non-finite component leaves the scan's records as they are and sets the scan's status word to 1
 * (the RSX_MOCOMP_STATUS_ANGLE rule); a motion that is exactly (0, 0, 0) copies the records: the input's bytes.
 * Tracker with rsx_cfear_track_params.compensate = 1 (rsx_cfear_tracker_push_timed only; P, M and the ring as above, comp(records,
 * M) the compensation just described).  Compensating with the PREDICTED motion alone is unstable (an error of the motion
 * becomes an error of the compensation and then of the next motion), so every scan is registered twice:
 *   scan 0   the first keyframe, as measured; the state remembers that (`first`) and keeps the scan's times
 *   scan i   pass 1: C0 = comp(scan, M), registered against the ring from the start pose of the rule above -> reg1
 *     reg1 status 1, 2, 4, 5: the failure rule above with C0 as the scan; `first` is cleared; reg = reg1
 *     reg1 status 0, 8: P1 = its pose, M1 = P^-1 o P1.  If `first`: the ring's only keyframe becomes comp(its records, its times,
 *       M1) at its pose, is binned again, and `first` is cleared.  C1 = comp(scan, M1); pass 2: C1 registered against the ring
 *       from P1 -> reg2
 *         reg2 status 0, 8: M = P^-1 o P2, P = P2; the keyframe decision above, with C1 as the keyframe's records
 *         reg2 fails: P = P1, M = M1, and C1 becomes the ring's only entry at P1 (flag 2)
 *       reg = reg2 in both cases, with reg.reserved = the iterations of pass 1
 * The scan is compensated once per pass, outside the Gauss-Newton loop.  As without compensation, results depend neither on how
 * a sequence is cut into pushes (the cut between scan 0 and scan 1 included) nor on how many sequences run side by side. */
/* rsx_cfear_surface_points_batch plus rows (int32 per point, checked to lie in [0, n_rows): RSX_ERR_BAD_ARG otherwise) and out_tau
 * (one float per record slot, laid out like out_records: scan i's at out_tau + i * max_records) */
int rsx_cfear_surface_points_timed_batch(rsx_cfear *h, const float *xy, const int32_t *rows, int32_t n_rows, const int64_t *offsets,
                                         int32_t n_scans, const rsx_cfear_params *params, rsx_cfear_surface_point *out_records,
                                         float *out_tau, int32_t max_records, int32_t *out_counts, int32_t *out_status);
/* device buffers, asynchronous on `stream`, no allocation; offsets and rows are trusted (a row outside [0, n_rows) gives a
 * meaningless time, nothing else) */
int rsx_cfear_surface_points_timed_batch_device(rsx_cfear *h, const float *d_xy, const int32_t *d_rows, int32_t n_rows,
                                                const int64_t *d_offsets, int32_t n_scans, const rsx_cfear_params *params,
                                                rsx_cfear_surface_point *d_records, float *d_tau, int32_t max_records, int32_t *d_counts,
                                                int32_t *d_status, void *stream);
/* n_scans scans in the ragged layout: scan i owns records (and times) [offsets[i], offsets[i + 1]) and is compensated with
 * motion[3 i ..]; out_status[i] (may be NULL) 0 or 1.  out_records may be records.  Host buffers, synchronous.  One launch, one
 * thread per record. */
int rsx_cfear_compensate_batch(rsx_cfear *h, const rsx_cfear_surface_point *records, const float *tau, const int64_t *offsets,
                               int32_t n_scans, const double *motion, rsx_cfear_surface_point *out_records, int32_t *out_status);
/* device buffers, asynchronous on `stream`, no allocation; offsets trusted */
int rsx_cfear_compensate_batch_device(rsx_cfear *h, const rsx_cfear_surface_point *d_records, const float *d_tau, const int64_t *d_offsets,
                                      int32_t n_scans, const double *d_motion, rsx_cfear_surface_point *d_out_records,
                                      int32_t *d_out_status, void *stream);
/* rsx_cfear_tracker_push with the records' times (tau[j] beside records[j]).  compensate = 0: rsx_cfear_tracker_push's bytes (tau
 * is not read).  rsx_cfear_tracker_push itself refuses compensate = 1 (RSX_ERR_BAD_ARG) */
int rsx_cfear_tracker_push_timed(rsx_cfear_tracker *h, const rsx_cfear_surface_point *records, const float *tau, const int64_t *offsets,
                                 const int32_t *n_scans, const rsx_cfear_params *params, const rsx_cfear_track_params *track,
                                 rsx_cfear_track_result *out);
int rsx_cfear_tracker_push_timed_device(rsx_cfear_tracker *h, const rsx_cfear_surface_point *d_records, const float *d_tau,
                                        const int64_t *d_offsets, const int32_t *d_n_scans, const rsx_cfear_params *params,
                                        const rsx_cfear_track_params *track, rsx_cfear_track_result *d_out, void *stream);

/* ============================== CorAl alignment quality ================================
 * How well two clouds are aligned, judged without any solver's residual (Adolfsson et al., "CorAl: Introspection for robust
 * radar and lidar perception in diverse environments using differential entropy"): if two clouds are aligned, merging them does
 * not blur the scene.  Per point, the differential entropy of the local point distribution in the merged cloud (joint) is compared
 * with the one in the point's own cloud (separate); quality = mean joint - mean separate entropy is about 0 when aligned and grows
 * with misalignment.  rsx_cfear_result.cost and rsx_icp_result.fitness are small wherever their solver found a minimum, right or
 * wrong; this measure depends on no solver and judges every estimator here alike.  CorAl's own code is not part of the reference
 * checkout: the rules below are restated in tests/coral_np.py, which is the arithmetic contract -- parity unpinned.
 * One job: cloud A (n_a <= RSX_CORAL_MAX_POINTS points, float x, y, A's frame), cloud B (n_b points, B's frame), T = six doubles
 * (r00, r01, tx, r10, r11, ty) taking B into A's frame -- a matrix, not a yaw: the device evaluates no sine.  All in fp64 on the
 * float inputs, nothing fused, every sum sequential in the order stated:
 *   - the joint cloud: joint index i < n_a is A's point i; n_a + k is B's point k moved, x' = (r00 bx + r01 by) + tx,
 *     y' = (r10 bx + r11 by) + ty, each rounded to float once, from there on an ordinary float input
 *   - the cell grid is CFEAR's: ix = floor(x / r), iy = floor(y / r) on 128 x 128 cells; a point with ix or iy outside [-64, 64)
 *     (non-finite included) is ignored by everything and sets RSX_CORAL_STATUS_RANGE; the others are valid
 *   - the walk of a valid point p: the 3 x 3 block of cells around p's cell, dy = -1, 0, 1 outer, dx = -1, 0, 1 inner, ascending
 *     joint index inside a cell, cells off the grid skipped; a visited q is a neighbour iff |q - p|^2 <= r^2 (p is its own
 *     neighbour).  The joint set: all neighbours in walk order; the separate set: those from p's own cloud, in the same order
 *   - pass 1: the counts m_joint and m_separate and the coordinate sums of both sets; p is SCORED iff m_separate >= min_points
 *     and m_joint - m_separate >= min_other (CorAl's "overlap only" rule)
 *   - pass 2 (scored points, each set): mu = sum / m; sxx += ex ex, syy += ey ey, sxy += ex ey with e = q - mu in walk order,
 *     each divided by (m - 1); det = sxx syy - sxy sxy
 *   - the per-point records (joint-index order) equal the restatement's bit for bit: the counts for every valid point, the
 *     determinants 0.0 for an unscored one, every field 0 for an invalid one
 *   - h(det) = 0.5 log(max(det, det_min)) + (1 + log(2 pi)); h_joint and h_separate are the means of h over the scored points,
 *     quality = h_joint - h_separate.  The logarithm and the order in which the per-point terms are added are the device's own
 *     (a fixed order: a job's result does not depend on its place in a batch); they are the only part that is not bit-exact
 * det_min: 1e-6 m^4 is of the order of the square of one range bin's area; it keeps a collinear neighbourhood from giving -inf. */

typedef struct rsx_coral rsx_coral;

#define RSX_CORAL_MAX_POINTS 8192 /* points of ONE cloud of a job (the joint cloud holds 16384) */
#define RSX_CORAL_STATUS_RANGE 1  /* some point of the joint cloud lay outside the 128 x 128 cell grid (or was not finite) */
#define RSX_CORAL_STATUS_POINTS 2 /* (device entries only) a cloud holds more than RSX_CORAL_MAX_POINTS points: nothing is computed,
                                     the result and the records are zero (the host entry refuses such a job with RSX_ERR_BAD_ARG) */
#define RSX_CORAL_STATUS_EMPTY 4  /* no point was scored: quality, h_joint and h_separate are 0 */

typedef struct {
  double radius;      /* r: cell side and neighbourhood radius [m], > 0 (3.5) */
  double det_min;     /* floor of a covariance determinant [m^4], > 0 (1e-6) */
  int32_t min_points; /* neighbours of its own cloud a scored point needs, >= 2 (6) */
  int32_t min_other;  /* neighbours of the other cloud a scored point needs, >= 0 (1) */
} rsx_coral_params;

typedef struct {
  double det_separate, det_joint; /* 0.0 unless the point is scored */
  int32_t m_separate, m_joint;    /* neighbours in its own cloud / in the joint cloud (itself included); 0 for an invalid point */
} rsx_coral_point;                /* 24 bytes */

typedef struct {
  double quality;     /* h_joint - h_separate */
  double h_joint;     /* mean joint entropy of the scored points */
  double h_separate;  /* mean separate entropy of the scored points */
  int32_t n_scored;   /* scored points of both clouds */
  int32_t n_scored_a; /* those of cloud A */
  int32_t n_valid;    /* points of the joint cloud inside the grid */
  int32_t status;     /* RSX_CORAL_STATUS_* */
} rsx_coral_result;   /* 40 bytes */

/* a violated rule of rsx_coral_params gives RSX_ERR_BAD_ARG in every entry that takes the struct (NULL = the defaults) */
int rsx_coral_default_params(rsx_coral_params *p);
int rsx_coral_create(int device, rsx_coral **out);
int rsx_coral_destroy(rsx_coral *h);
/* n_jobs jobs; job i owns points [a_offsets[i], a_offsets[i + 1]) of a_xy and [b_offsets[i], b_offsets[i + 1]) of b_xy (float x, y
 * per point) and transforms[6 i .. 6 i + 5] (transforms NULL: every job at the identity); both offset arrays as for
 * rsx_orora_register_batch (checked), and no cloud may hold more than RSX_CORAL_MAX_POINTS points (RSX_ERR_BAD_ARG).
 * out_results[i] is job i's result; out_points (may be NULL) receives the records, job i's from a_offsets[i] + b_offsets[i] on.
 * Host buffers, synchronous.  One workgroup per job, one launch. */
int rsx_coral_quality_batch(rsx_coral *h, const float *a_xy, const int64_t *a_offsets, const float *b_xy, const int64_t *b_offsets, int32_t n_jobs,
                            const double *transforms, const rsx_coral_params *params, rsx_coral_result *out_results,
                            rsx_coral_point *out_points);
/* device buffers (d_transforms and d_points too, or NULL), asynchronous on `stream`; a point is point_stride floats (>= 2), x and
 * y first, so a packed float4 cloud is read in place (point_stride 4); the offsets are trusted, a job with a cloud above the cap
 * gets RSX_CORAL_STATUS_POINTS.  The handle's workspace grows to min(n_jobs, 256) x 128 KiB; no allocation otherwise */
int rsx_coral_quality_batch_device(rsx_coral *h, const float *d_a, const int64_t *d_a_offsets, const float *d_b, const int64_t *d_b_offsets,
                                   int32_t point_stride, int32_t n_jobs, const double *d_transforms, const rsx_coral_params *params,
                                   rsx_coral_result *d_results, rsx_coral_point *d_points, void *stream);

/* ============================== phase-correlation registration ========================
 * Dense, correspondence-free registration of two polar scans (Fourier-Mellin at scale 1; Checchin et al., "Radar scan matching
 * SLAM using the Fourier-Mellin transform"; Park et al., "PhaRaO"): the one estimator here that reads the power image itself, so
 * it needs no detector, no matches and no start value.  None of this is in the reference checkout: the rules below are restated
 * in tests/phasecorr_np.py, which is the arithmetic contract -- parity unpinned.
 * Frames: azimuth 0 is +x (forward), a return at azimuth phi and range rho sits at (rho cos phi, rho sin phi); image column j is
 * x = (j - N/2) resolution, image row i is y = (i - N/2) resolution.  The result of a pair (src, dst) is the transform taking src
 * into dst's frame, p_dst = R(theta) p_src + (x, y) -- the convention of rsx_cfear_result.  The azimuth rows are taken as EVENLY
 * SPACED, row a at 2 pi a / rows; an uneven encoder grid is out of scope.
 *   1. tables, made by the host in fp64 and rounded once to fp32, one set per handle: the resampling map (for every pixel of the
 *      N x N grid the range-bin coordinate rho / range_resolution - 0.5 and the azimuth-row coordinate; a pixel with
 *      rho > (N/2 - 1) resolution, or a range coordinate below min_range_bins or above cols - 1, is marked and reads 0), the Hann
 *      window 0.5 - 0.5 cos(2 pi k / N), the table of cos and sin of 2 pi k / N (mirror-symmetric bit for bit), the N directions
 *      of the polar resampling and cos(pi xi) of the high-pass
 *   2. the windowed Cartesian image at rotation psi: azimuth coordinate = map + psi / azimuth step, wrapped to [0, rows); a
 *      bilinear blend of four u8 samples; times hann[i], times hann[j].  fp32 in the operation order tests/phasecorr_np.py states:
 *      BIT-IDENTICAL to the restatement
 *   3. per scan, at psi = 0: the 2-D FFT F; its magnitude, fftshifted, times (1 - X)(2 - X) with X = cos(pi xi) cos(pi eta);
 *      resampled bilinearly at N angles over [0, pi) x radii 4 .. N/2 - 1; a 1-D FFT along the angle for every radius.  Both
 *      spectra stay in the handle's slot of the scan: every image of a batch is transformed once, whatever number of pairs reads it
 *   4. rotation of a pair: C = A_dst conj(A_src), C / (|C| + 1e-9 max|C|), summed over the radii in ascending order -- radius r
 *      contributes its angular frequencies |f| <= r only (above, the resampled ring holds the kinks of the interpolant, which belong
 *      to the grid and vote for a rotation of 0) -- inverse 1-D FFT, divided by the sum of the terms' magnitudes (each about 1),
 *      so the curve is 1 at a perfect match whatever the 1e-9 removes; the peak (ties: the lowest index) and a three-point parabola
 *      give theta0 in [-pi/2, pi/2), known modulo pi
 *   5. translation, for theta0 and (resolve_half_turn) theta0 + pi: the image of src at psi = -theta, its 2-D FFT G,
 *      C = F_dst conj(G), C / (|C| + 1e-9 max|C|), inverse 2-D FFT over the sum of the terms' magnitudes (1 at a perfect match,
 *      as above); the peak (ties: the lowest row-major index), a three-point
 *      parabola per axis; the candidate with the higher peak wins (a tie: theta0).  peak_ratio = the largest value outside the
 *      peak's 3 x 3 neighbourhood (wrapped) over the peak
 * The three values under each parabola are sums of the inverse transform taken directly, in fp64 over the fp32 cross-power in
 * index order: with the mirror-symmetric table a pair of a scan with itself gives x = y = theta = 0 exactly.  All transforms are
 * fp32 in a fixed order, every maximum breaks ties by index, no float atomics: a pair's result does not depend on its place in
 * the batch or on the batch's size.  The angles stay in device memory between the steps: a batch is nine launches and no host
 * round trip, whatever its size.
 * Defaults N = 256 at 0.5 m per pixel, from a sweep through the restatement on synth.polar_sequence(3, 6), five consecutive pairs
 * (largest translation and rotation error, largest peak_ratio, smallest peak and rot_peak):
 *     N    m/pixel   error [m]  [rad]    peak_ratio  peak   rot_peak
 *     64   2.0       19.2       3.04     0.87        0.07   0.12     (wrong peaks)
 *     64   1.0       0.45       0.054    0.73        0.15   0.13
 *     128  1.0       0.26       0.016    0.21        0.21   0.10
 *     128  0.5       0.083      0.0093   0.14        0.29   0.13
 *     256  0.5       0.086      0.0016   0.062       0.43   0.21     (default)
 *     256  0.25      0.030      0.0030   0.22        0.20   0.16
 *     512  0.25      0.035      0.0008   0.087       0.24   0.18
 * N = 64 does not register this drive; it registers pure rotations of one scene (by 0, 1, 100, 200, 333 rows of 400, at 2 m per
 * pixel: within 0.81 angle bin; N = 256: within 0.36) and is the smallest size the transforms are built for. */

typedef struct rsx_phasecorr rsx_phasecorr;

#define RSX_PHASECORR_STATUS_ROTATION 1 /* |theta| > max_rotation: the result is reported as found */
#define RSX_PHASECORR_STATUS_INDEX 2    /* (device entry only) a pair names an image outside the batch: nothing is computed, the
                                           result is zero (the host entry refuses such a batch with RSX_ERR_BAD_ARG) */

typedef struct {
  int32_t n;                 /* image size N: 64, 128, 256 or 512 (256) */
  int32_t min_range_bins;    /* range coordinates below it read 0, >= 0 (58: the keypoint extractors' min_range) */
  double resolution;         /* metres per pixel, > 0 (0.5) */
  double range_resolution;   /* metres per range bin, > 0 (0.0595) */
  double max_rotation;       /* [rad] a pair with |theta| above it gets RSX_PHASECORR_STATUS_ROTATION; 0 = unlimited (0) */
  int32_t resolve_half_turn; /* also try theta0 + pi (1) */
  int32_t reserved;          /* 0 */
} rsx_phasecorr_params;      /* 40 bytes */

typedef struct {
  double x, y, theta;   /* p_dst = R(theta) p_src + (x, y); metres, rad in (-pi, pi] */
  double peak;          /* the translation surface at its peak (1 = identical images) */
  double peak_ratio;    /* runner-up outside the peak's 3 x 3 neighbourhood / peak: small = unambiguous */
  double rot_peak;      /* the rotation curve at its peak */
  int32_t half_turn;    /* 1: theta0 + pi won */
  int32_t status;       /* RSX_PHASECORR_STATUS_* */
} rsx_phasecorr_result; /* 56 bytes */

/* a violated rule of rsx_phasecorr_params gives RSX_ERR_BAD_ARG in every entry that takes the struct (NULL = the defaults): N not
 * one of the four sizes, a resolution that is not positive and finite, a negative min_range_bins or max_rotation, and a disc that
 * does not fit the scan: (N / 2) resolution > (cols - 1) range_resolution */
int rsx_phasecorr_default_params(rsx_phasecorr_params *p);
/* one handle per image shape (rows 1 .. 4096 azimuths x cols 2 .. 8192 range bins) and parameter set; the tables are made here */
int rsx_phasecorr_create(int device, int32_t rows, int32_t cols, const rsx_phasecorr_params *params, rsx_phasecorr **out);
int rsx_phasecorr_destroy(rsx_phasecorr *h);
/* n_images host images image_stride_bytes apart, rows x row_stride bytes each, power samples at [col_offset, col_offset + cols) of
 * a row; pairs: n_pairs x (src, dst) int32 image indices (checked: RSX_ERR_BAD_ARG outside [0, n_images)).  out_results[n_pairs];
 * out_cart (may be NULL) receives the psi = 0 image of every scan, [n_images][N][N] floats.  Host buffers, synchronous. */
int rsx_phasecorr_register_batch(rsx_phasecorr *h, const uint8_t *imgs, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride,
                                 int32_t col_offset, const int32_t *pairs, int32_t n_pairs, rsx_phasecorr_result *out_results, float *out_cart);
/* the same on device buffers, asynchronous on `stream`, no host synchronisation; a pair with an index outside the batch gets
 * RSX_PHASECORR_STATUS_INDEX.  No allocation beyond the handle's workspace, which grows to
 *   n_images (12 N^2 - 32 N) + n_pairs (40 N^2 + 2048 + 4 N) + 64 bytes
 * (per scan F and the angle spectrum; per pair, for both candidates, G, the column-transformed cross-power and the surface, the
 * partial maxima and sums, the rotation curve) and is kept between calls: 0.75 MiB per scan and 2.5 MiB per pair at N = 256. */
int rsx_phasecorr_register_batch_device(rsx_phasecorr *h, const uint8_t *d_imgs, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride,
                                        int32_t col_offset, const int32_t *d_pairs, int32_t n_pairs, rsx_phasecorr_result *d_results,
                                        float *d_cart, void *stream);

/* ============================== radar scan context ====================================
 * The "radar scan context" of the MulRan paper (Kim et al., ICRA 2020; reference README.md:28-29): the 20 x 60 polar grid
 * of the ScanContext descriptor filled with received power straight from the polar image -- dense where the descriptors of
 * the z = 0 keypoint cloud are binary, no keypoint extractor involved.  MulRan's own builder is not part of the reference
 * checkout: the rule below is restated in tests/radarsc_np.py, which is the arithmetic contract -- parity unpinned.
 *   ring    of range bin j (SC.cpp:175,178, fp64): r = (j + 0.5) * (double)resolution; none when j < min_range or
 *           r > max_radius, else max(min(20, (int)ceil(r / max_radius * 20)), 1) - 1
 *   sector  of azimuth row a (SC.cpp:179, fp64): th = (double)az[a] * 57.29577951308232, t = th / 360 - floor(th / 360),
 *           max(min(60, (int)ceil(t * 60)), 1) - 1; none when az[a] is not finite.  The grid need not increase or lie in
 *           [0, 2 pi)
 *   sample  v = max(p - power_floor, 0) on integers
 *   cell    RSX_RADARSC_MEAN: (float)((double)sum / (double)count) over every sample of the cell (integer sum), 0 when empty;
 *           RSX_RADARSC_MAX: (float)max, 0 when empty
 * Integer sums: a descriptor does not depend on the order of the reduction and equals the restatement bit for bit.
 * Output: "f32 sector-major", 1200 floats per scan -- what rsx_sc_add_descriptors_f32_device and rsx_sc_query_device take.
 * One launch per batch; per 400 x 3360 scan the kernel reads the 0.51 MB between min_range and the last bin inside
 * max_radius and writes 4.8 kB.  Image and azimuth arguments as for rsx_cen2019_extract_batch; the azimuths are required. */

typedef struct rsx_radarsc rsx_radarsc;

#define RSX_RADARSC_MEAN 0
#define RSX_RADARSC_MAX 1

typedef struct {
  double max_radius;   /* outer edge of ring 19 [m] (80: SC.h:87 PC_MAX_RADIUS); positive, finite */
  float resolution;    /* metres per range bin (0.0595); positive */
  int32_t min_range;   /* first range bin used (58); >= 0 */
  int32_t power_floor; /* subtracted from every sample, clamped at 0 (0); 0 .. 255 */
  int32_t stat;        /* RSX_RADARSC_MEAN (default) or RSX_RADARSC_MAX */
} rsx_radarsc_params;

int rsx_radarsc_default_params(rsx_radarsc_params *p);
/* one handle per image shape (rows 1 .. 4096 azimuths x cols 1 .. 8192 range bins) and parameter set (NULL: the defaults);
 * anything else is RSX_ERR_BAD_ARG */
int rsx_radarsc_create(int device, int32_t rows, int32_t cols, const rsx_radarsc_params *params, rsx_radarsc **out);
int rsx_radarsc_destroy(rsx_radarsc *h);
/* n_images host images -> out_descs [n_images][1200].  Synchronous. */
int rsx_radarsc_build_batch(rsx_radarsc *h, const uint8_t *imgs, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride,
                            int32_t col_offset, const float *azimuths, int32_t azimuths_per_image, float *out_descs);
/* device buffers, asynchronous on `stream`: one launch, no host synchronisation, the (per-image) grids are read on the
 * device.  Only bytes inside each image's rows x row_stride bytes are read, whatever the alignment of d_imgs. */
int rsx_radarsc_build_batch_device(rsx_radarsc *h, const uint8_t *d_imgs, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride,
                                   int32_t col_offset, const float *d_azimuths, int32_t azimuths_per_image, float *d_descs, void *stream);
/* build + insert without leaving the GPU: the descriptors of n_images device images become the next n_images keyframes of
 * the database (a sharded handle keeps those of its residue class; every rank calls this with every scan, as for
 * rsx_sc_add_points).  Both handles on the same device. */
int rsx_sc_add_polar_batch_device(rsx_sc *h, rsx_radarsc *rc, const uint8_t *d_imgs, int32_t n_images, int64_t image_stride_bytes,
                                  int32_t row_stride, int32_t col_offset, const float *d_azimuths, int32_t azimuths_per_image, void *stream);
/* one host image (rows x row_stride bytes) and its grid (rows floats); out_index (optional) = its global keyframe index */
int rsx_sc_add_polar(rsx_sc *h, rsx_radarsc *rc, const uint8_t *img, int32_t row_stride, int32_t col_offset, const float *azimuths,
                     int32_t *out_index);

/* ============================== radar grid map ========================================
 * Polar scans at known poses accumulated into a fixed, georeferenced cell grid: the radar mosaic (mean received power per
 * cell) and, for whatever plans on it, how often a cell returned a strong echo.  The one dense product of the library; also
 * the one place where the poses can be judged by eye (a mosaic built at wrong poses is blurred: tests/test_gridmap_restatement.py
 * measures it).  None of this is in the reference checkout: the rule below is restated in tests/gridmap_np.py, which is the
 * arithmetic contract -- parity unpinned.
 * State: three uint32 planes [height][width], row-major with row = y: `sum` of the samples a cell received, `cnt` the number of
 * scans that observed it, `hit` the number of those whose sample was >= hit_threshold.  Integers only: the map does not depend
 * on the order of the scans, on how a sequence is cut into batches or on the order of any reduction, and equals the restatement
 * byte for byte.  (A plane wraps at 2^32: 16.8 million saturated observations of one cell.)
 * Frames: azimuth 0 is +x, a return at azimuth phi and range rho sits at (rho cos phi, rho sin phi) in the sensor frame
 * (rsx_phasecorr's convention); the azimuth rows are taken as EVENLY SPACED, row a at 2 pi a / rows (an uneven encoder grid is
 * out of scope).  A scan's pose is six doubles r00, r01, tx, r10, r11, ty taking the sensor frame into the map frame,
 * m = R p + t -- rsx_coral's transform, a matrix and not a yaw: the device evaluates no sine.  The matrix is taken as a rotation
 * and not checked (the list of the tiles a scan can reach allows for one within 1e-7 of a rotation).
 * Tables, made by the host at create in fp64 and rounded once to fp32: c[a] = cos(2 pi a / rows), s[a] = sin(2 pi a / rows),
 * widened back to fp64 where used.
 * Per (scan, cell (ix, iy)), fp64 on plain operations, nothing fused:
 *   1. the cell centre mx = origin_x + (ix + 0.5) resolution, my = origin_y + (iy + 0.5) resolution
 *   2. dx = mx - tx, dy = my - ty
 *   3. px = r00 dx + r10 dy, py = r01 dx + r11 dy                      (the transposed matrix: map frame into sensor frame)
 *   4. d2 = px px + py py
 *   5. the range bin j with (j rr)^2 <= d2 < ((j + 1) rr)^2, j rr formed in fp64 and squared (bin j covers [j rr, (j + 1) rr):
 *      rsx_radarsc's centre (j + 0.5) rr); the cell is NOT OBSERVED when j < min_range_bins, when j >= cols, or (max_range > 0)
 *      when d2 > max_range^2
 *   6. the azimuth row a that maximises c[a] px + s[a] py (the nearest beam); among equal rows the smallest a
 *   7. the sample v = the maximum of the power bytes of row a at bins j - range_halfwidth .. j + range_halfwidth, bins below
 *      min_range_bins or above cols - 1 left out
 *   8. cnt += 1, sum += v, hit += (v >= hit_threshold)
 * The kernel finds j and a from fp32 guesses and confirms them by the comparisons above: the guesses never show.  Cells outside
 * the map do not exist; a scan whose footprint misses the map changes nothing.
 * Render, on integers: RSX_GRIDMAP_MEAN gives uint8 (2 sum + cnt) / (2 cnt), 0 where cnt < min_observations; RSX_GRIDMAP_HITS
 * gives int8 in the convention of nav_msgs/OccupancyGrid, -1 where cnt < min_observations, else (200 hit + cnt) / (2 cnt), which
 * lies in 0 .. 100.  min_observations >= 1.
 * One launch per call whatever the batch: one workgroup per 32 x 32 tile of the map lists the scans that can reach it (a circle
 * against the box of its cell centres) and keeps its cells' accumulators in registers over the batch; no atomics, a tile's planes
 * are read and written once per call.
 * hit_threshold 120 is a value for the synthetic drive only (no real radar data has been seen).  Share of the cells seen by all
 * six scans of synth.polar_sequence(11, 6) (1024 x 1024 cells of 0.5 m, the scans at their true poses) with at least half of
 * their observations a hit, from tests/gridmap_np.py:
 *     range_halfwidth   threshold 60    90      120     150
 *     4                 0.58            0.36    0.27    0.21
 *     0                 0.26            0.18    0.13    0.09        (493163 cells)
 * The drive's world is dense, and a 1.8 degree beam is nine cells wide at 150 m. */

typedef struct rsx_gridmap rsx_gridmap;

#define RSX_GRIDMAP_MEAN 0
#define RSX_GRIDMAP_HITS 1
#define RSX_GRIDMAP_STATUS_TRANSFORM 1 /* (device entry only) the scan's transform holds a non-finite entry: the scan is skipped
                                          (the host entry refuses such a batch with RSX_ERR_BAD_ARG) */

typedef struct {
  int32_t width, height;    /* cells; each 64 .. 8192 and a multiple of 64 (1024 x 1024) */
  double resolution;        /* metres per cell, > 0 (0.5) */
  double origin_x, origin_y; /* map coordinates of the outer corner of cell (0, 0) (-256, -256) */
  double range_resolution;  /* metres per range bin, > 0 (0.0595) */
  double max_range;         /* [m] cells farther than this are not observed; 0 = to the last bin (0) */
  int32_t min_range_bins;   /* first range bin used, >= 0 (58: the keypoint extractors' min_range) */
  int32_t range_halfwidth;  /* bins either side of j that the sample is the maximum of, 0 .. 8192 (4 = floor(resolution /
                               (2 range_resolution)): a cell is as deep as 8.4 bins) */
  int32_t hit_threshold;    /* sample level that counts as a hit, 0 .. 255 (120: see the table above) */
  int32_t reserved;         /* 0 */
} rsx_gridmap_params;       /* 64 bytes */

/* a violated rule of rsx_gridmap_params gives RSX_ERR_BAD_ARG, judged before the device is looked at */
int rsx_gridmap_default_params(rsx_gridmap_params *p);
/* one handle per image shape (rows 1 .. 4096 azimuths x cols 2 .. 8192 range bins) and parameter set (NULL: the defaults);
 * allocates and zeroes the planes (12 bytes per cell), makes the tables */
int rsx_gridmap_create(int device, int32_t rows, int32_t cols, const rsx_gridmap_params *params, rsx_gridmap **out);
int rsx_gridmap_destroy(rsx_gridmap *h);
/* zeroes the planes; asynchronous on `stream` */
int rsx_gridmap_clear(rsx_gridmap *h, void *stream);
/* n_images host images (image arguments as for rsx_radarsc_build_batch) at transforms[6 i .. 6 i + 5] into the planes.  A
 * non-finite transform entry refuses the whole batch (RSX_ERR_BAD_ARG, nothing added).  Host buffers, synchronous. */
int rsx_gridmap_add_batch(rsx_gridmap *h, const uint8_t *imgs, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride,
                          int32_t col_offset, const double *transforms);
/* device buffers, asynchronous on `stream`: one launch, no host synchronisation, no allocation.  A scan with a non-finite transform
 * is skipped; d_status (may be NULL) receives per scan 0 or RSX_GRIDMAP_STATUS_TRANSFORM.  Only bytes inside each image's
 * rows x row_stride bytes are read, whatever the alignment of d_imgs. */
int rsx_gridmap_add_batch_device(rsx_gridmap *h, const uint8_t *d_imgs, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride,
                                 int32_t col_offset, const double *d_transforms, int32_t *d_status, void *stream);
/* the window [x, x + w) x [y, y + hgt) of the planes to host arrays [hgt][w]; any pointer may be NULL; a window that is empty or
 * not inside the map is RSX_ERR_BAD_ARG.  Synchronous. */
int rsx_gridmap_read(rsx_gridmap *h, int32_t x, int32_t y, int32_t w, int32_t hgt, uint32_t *out_sum, uint32_t *out_cnt, uint32_t *out_hit);
/* the planes in device memory ([height][width] uint32, pitch_bytes = 4 width apart), for callers that stay on the GPU; any
 * pointer may be NULL.  Valid until the handle is destroyed; the caller orders its reads behind the handle's calls. */
int rsx_gridmap_planes_device(rsx_gridmap *h, uint32_t **d_sum, uint32_t **d_cnt, uint32_t **d_hit, int64_t *pitch_bytes);
/* a window rendered to a host array [hgt][w] of bytes (uint8 for RSX_GRIDMAP_MEAN, int8 for RSX_GRIDMAP_HITS).  Synchronous. */
int rsx_gridmap_render(rsx_gridmap *h, int32_t mode, int32_t min_observations, int32_t x, int32_t y, int32_t w, int32_t hgt, void *out);
/* the same into a device buffer, asynchronous on `stream` */
int rsx_gridmap_render_device(rsx_gridmap *h, int32_t mode, int32_t min_observations, int32_t x, int32_t y, int32_t w, int32_t hgt, void *d_out,
                              void *stream);

/* ---- localising a point cloud in the map: correlative scan-to-map matching (Olson 2009; Cartographer's real-time correlative
 * matcher), exhaustive over a window of rotations and whole-cell shifts around a prior pose.  None of this is in the reference
 * checkout: the rule below is restated in tests/gridmatch_np.py, which is the arithmetic contract -- parity unpinned.  Integers
 * from step 5 on: the scores equal the restatement byte for byte and do not depend on the order of any sum.
 * The likelihood plane: uint8 [height][width], a frozen snapshot that matching reads (the planes may go on accumulating).  It is
 * allocated at the first rsx_gridmap_likelihood_* call, (height + 256) x (width + 256) bytes: the plane in a zeroed frame of 128
 * cells, which is why its pitch is not its width.  rsx_gridmap_likelihood_update fills it from the planes: with RSX_GRIDMAP_MEAN
 * the byte that render gives, with RSX_GRIDMAP_HITS render's value with -1 replaced by 0 (0 .. 100).  rsx_gridmap_likelihood_set
 * loads any image, a mosaic saved in an earlier session for one.
 * A job: the points [offsets[i], offsets[i + 1]) of a float x, y array (rsx_coral's ragged convention: offsets[0] == 0, none
 * below the one before it; at most RSX_GRIDMAP_MATCH_MAX_POINTS points) and a prior pose, six doubles r00 r01 tx r10 r11 ty taking
 * the cloud's frame into the map frame.
 * Candidates: the triples (k, v, u), |k| <= K = angle_steps, |v| <= V = y_cells, |u| <= U = x_cells; linear index
 * ((k + K)(2V + 1) + (v + V))(2U + 1) + (u + U).
 * Tables, made by the host per call in fp64 and rounded once to fp32: c[k] = cos(k angle_step), s[k] = sin(k angle_step), the
 * angle formed as (double)k * angle_step; widened back to fp64 where used.  inv_res = 1.0 / resolution, on the host.
 * Per (job, k, point (x, y)), fp64 on plain operations, nothing fused:
 *   1. rx = c x - s y, ry = s x + c y
 *   2. mx = r00 rx + r01 ry + tx, my = r10 rx + r11 ry + ty                      (left to right)
 *   3. fx = (mx - origin_x) inv_res, fy = (my - origin_y) inv_res
 *   4. the point is PLACED iff fx >= -64 && fx < width + 64 && fy >= -64 && fy < height + 64 (a non-finite point fails this and
 *      is skipped; no candidate can reach a point that is not placed)
 *   5. ix = (int)floor(fx), iy = (int)floor(fy)
 * score(k, v, u) = the sum of L[iy + v][ix + u] over the placed points whose shifted cell is inside the map: a uint32, at most
 * 8192 * 255.
 * The winner is the highest score; among equal scores the smallest |k|, then the smallest u u + v v, then the smallest linear index.
 * Result: transform = R_prior Rot(k) with the table values of the winner's k,
 *     r00' = r00 c + r01 s, r01' = r01 c - r00 s, r10' = r10 c + r11 s, r11' = r11 c - r10 s,
 *     tx' = tx + (double)u resolution, ty' = ty + (double)v resolution;
 * score_prior = score(0, 0, 0); score_runner_up = the best score among the candidates farther than 1 from the winner in at least
 * one of k, u, v (0 if there is none): peak_ratio's counterpart; n_points = the points placed at the winner's k, n_inside = those
 * of them whose cell shifted by the winner's (u, v) is inside the map.
 * Status: RSX_GRIDMAP_MATCH_STATUS_TRANSFORM, a prior with a non-finite entry: the job is skipped, its result is zero but for the
 * status, its scores are zero.  _POINTS (device entry only; the host entry refuses the batch with RSX_ERR_BAD_ARG): more than the
 * cap of points, treated like _TRANSFORM.  _EMPTY: the winning score is 0 (then k = u = v = 0): transform = the prior, unchanged.
 * Two launches per call whatever the batch: one workgroup per (job, k) puts the cells of the rotated cloud into LDS and sums,
 * every thread four neighbouring u of one v from one unaligned 32-bit read per point; one workgroup per job then picks the winner
 * with an index-carrying key.  No atomics on device memory. */

#define RSX_GRIDMAP_MATCH_MAX_POINTS 8192
#define RSX_GRIDMAP_MATCH_STATUS_TRANSFORM 1
#define RSX_GRIDMAP_MATCH_STATUS_POINTS 2
#define RSX_GRIDMAP_MATCH_STATUS_EMPTY 4

typedef struct {
  double angle_step;    /* [rad] between two rotations; > 0 and finite when angle_steps > 0 (0.01) */
  int32_t angle_steps;  /* K: rotations -K .. K, 0 .. 64 (8) */
  int32_t x_cells;      /* U: shifts -U .. U cells along x, 0 .. 32 (8) */
  int32_t y_cells;      /* V: shifts -V .. V cells along y, 0 .. 32 (8) */
  int32_t reserved;     /* 0 */
} rsx_gridmap_match_params; /* 24 bytes */

typedef struct {
  double transform[6];      /* r00 r01 tx r10 r11 ty of the winner */
  int32_t k, u, v;          /* the winner */
  uint32_t score, score_prior, score_runner_up;
  int32_t n_points, n_inside;
  int32_t status;           /* RSX_GRIDMAP_MATCH_STATUS_* */
  int32_t reserved;         /* 0 */
} rsx_gridmap_match_result; /* 88 bytes */

/* a violated rule of rsx_gridmap_match_params gives RSX_ERR_BAD_ARG in every entry that takes the struct (NULL = the defaults),
 * judged before the handle or the device is looked at */
int rsx_gridmap_match_default_params(rsx_gridmap_match_params *p);
/* the likelihood plane from the planes as they stand: mode and min_observations as for render.  Asynchronous on `stream`, one
 * launch (the first rsx_gridmap_likelihood_* call of a handle also allocates the plane and zeroes its frame). */
int rsx_gridmap_likelihood_update(rsx_gridmap *h, int32_t mode, int32_t min_observations, void *stream);
/* the likelihood plane from a host image [height][width].  Synchronous. */
int rsx_gridmap_likelihood_set(rsx_gridmap *h, const uint8_t *img);
/* cell (0, 0) of the likelihood plane in device memory and the bytes from one row to the next (width + 256); allocates the plane
 * when no call has yet.  A caller that writes the plane itself writes [height][width] bytes at that pitch, ordered against the
 * handle's calls, and calls nothing else to make it count: handing out the pointer marks the plane as filled. */
int rsx_gridmap_likelihood_device(rsx_gridmap *h, uint8_t **d_likelihood, int64_t *pitch_bytes);
/* a window of the likelihood plane to a host array [hgt][w], as rsx_gridmap_read; RSX_ERR_BAD_ARG before any update or set.
 * Synchronous. */
int rsx_gridmap_likelihood_read(rsx_gridmap *h, int32_t x, int32_t y, int32_t w, int32_t hgt, uint8_t *out);
/* n_jobs jobs against the likelihood plane.  Host buffers, synchronous.  out_scores (may be NULL): the whole volume, uint32
 * [job][2K + 1][2V + 1][2U + 1].  The offsets are checked, a job above the cap refuses the batch; before any likelihood exists
 * the call is RSX_ERR_BAD_ARG and touches nothing.  Staged in sub-batches of at most 64 MB of volume (a job's bytes do not
 * depend on the cut). */
int rsx_gridmap_match_batch(rsx_gridmap *h, const float *xy, const int64_t *offsets, int32_t n_jobs, const double *priors,
                            const rsx_gridmap_match_params *params, rsx_gridmap_match_result *out_results, uint32_t *out_scores);
/* device buffers, asynchronous on `stream`: two launches, no host synchronisation; point i of the array is d_xy[point_stride i]
 * and d_xy[point_stride i + 1] (point_stride >= 2: a packed float4 cloud is read in place, whatever its alignment beyond 4
 * bytes); the offsets are trusted; a job above the cap gets RSX_GRIDMAP_MATCH_STATUS_POINTS.  n_jobs (2K + 1) < 2^31.
 * Workspace: with d_scores NULL the handle keeps the volume itself, a buffer that grows (to the next power of two) to
 * n_jobs (2K + 1)(2V + 1)(2U + 1) * 4 bytes and is never given back before destroy -- 19652 bytes per job at the defaults, 2.2 MB
 * per job at the largest window; with d_scores given nothing is allocated. */
int rsx_gridmap_match_batch_device(rsx_gridmap *h, const float *d_xy, const int64_t *d_offsets, int32_t point_stride, int32_t n_jobs,
                                   const double *d_priors, const rsx_gridmap_match_params *params, rsx_gridmap_match_result *d_results,
                                   uint32_t *d_scores, void *stream);

/* ---- the same search over a wide window, pruned by bounds (csrc/gridsearch.hip): re-localising after a lost track, starting in a
 * saved mosaic, placing a loop candidate that has a yaw and no translation.  Two levels, exact: the winner is the winner that the
 * exhaustive rule above would give over the same window; pruning changes the cost only.  Restated in tests/gridsearch_np.py, which
 * is the arithmetic contract -- parity unpinned; integers from the cell on, bytes equal to the restatement.
 * Jobs, priors, the ragged convention, the cap of points, the tables and steps 1 - 5 are those of rsx_gridmap_match_*, but for the
 * placement margin of step 4: PL = max(64, U, V) replaces 64 (fx >= -PL && fx < width + PL, likewise fy); with U, V <= 64 that is
 * the rule above.
 * Candidates (k, v, u), |k| <= K <= 180, |v| <= V <= 256, |u| <= U <= 256; score(k, v, u), the tie order and the linear index as above.
 * Pooled plane: P[y][x] = max of L[y + a][x + b] over 0 <= a, b < 8, for every integer y, x; cells outside the map count as 0.
 * Blocks: nbu = ceil((2U + 1) / 8), nbv = ceil((2V + 1) / 8); block (k, bv, bu) holds the candidates with v in
 * [-V + 8 bv, min(V, -V + 8 bv + 7)] and u likewise.  bound(k, bv, bu) = the sum over the placed points of
 * P[iy - V + 8 bv][ix - U + 8 bu], a uint32: no smaller than any score of the block.
 * Threshold: seed(k) = the highest score among the candidates of that block of k which has the highest bound (among equal bounds
 * the smallest bv nbu + bu); T0 = max(min_score, score(0, 0, 0), max over k of seed(k)).  A block is REFINED iff its bound >=
 * max(T0, 1): a block whose bound equals T0 stays, because a tie can win the order.
 * The winner is the best candidate by the tie order with score >= max(min_score, 1) among the refined blocks.  (The exhaustive
 * winner's score s* is >= T0 once it is eligible, and its block's bound >= s*: its block is refined.)
 * Result: transform, k, u, v, score, score_prior, n_points, n_inside as in rsx_gridmap_match_result; n_blocks = (2K + 1) nbv nbu;
 * n_refined = the number of refined blocks, by the rule above whatever the kernel skips on top; bound_runner_up = the largest bound
 * among the blocks farther than 1 from the winner's block in k, bv or bu (0 if there is none, or if status != 0): score >
 * bound_runner_up proves that nothing outside the neighbourhood of the winner's block comes near.
 * Status: _TRANSFORM and _POINTS as above (the record is zero but for the status).  _EMPTY: min_score == 0 and the best score is
 * 0: k = u = v = 0, transform = the prior bit for bit.  _BELOW: min_score > 0 and no candidate reaches it: k = u = v = 0, transform =
 * the prior, score = 0; score_prior, n_blocks, n_refined and the counts (at k = 0) still by the rule.
 * For K <= 64, U, V <= 32 and min_score 0 the fields transform, k, u, v, score, score_prior, n_points, n_inside and status equal
 * rsx_gridmap_match_batch's byte for byte.
 * Three launches per call whatever the batch (bounds and seeds, one workgroup per (job, k); refinement, likewise; the pick, one
 * workgroup per job); no atomics on device memory. */

#define RSX_GRIDMAP_SEARCH_STATUS_BELOW 8
#define RSX_GRIDMAP_SEARCH_MAX_CELLS 256
#define RSX_GRIDMAP_SEARCH_MAX_ANGLE_STEPS 180

typedef struct {
  double angle_step;    /* as rsx_gridmap_match_params (0.01) */
  int32_t angle_steps;  /* K: 0 .. 180 (32) */
  int32_t x_cells;      /* U: 0 .. 256 (64) */
  int32_t y_cells;      /* V: 0 .. 256 (64) */
  uint32_t min_score;   /* a winner must reach it; 0 = none (0) */
} rsx_gridmap_search_params; /* 24 bytes */

typedef struct {
  double transform[6];      /* r00 r01 tx r10 r11 ty of the winner */
  int32_t k, u, v;          /* the winner */
  uint32_t score, score_prior, bound_runner_up;
  int32_t n_points, n_inside;
  int32_t status;           /* RSX_GRIDMAP_MATCH_STATUS_* | RSX_GRIDMAP_SEARCH_STATUS_BELOW */
  int32_t n_blocks, n_refined;
  int32_t reserved;         /* 0 */
} rsx_gridmap_search_result; /* 96 bytes */

/* a violated rule of rsx_gridmap_search_params gives RSX_ERR_BAD_ARG in every entry that takes the struct (NULL = the defaults),
 * judged before the handle or the device is looked at */
int rsx_gridmap_search_default_params(rsx_gridmap_search_params *p);
/* what a search reads: a frozen snapshot of the likelihood plane as it stands (later likelihood changes are not seen until the next
 * prepare), good for searches with U, V <= max_cells (0 .. 256).  Two buffers of the search's own: a copy of the plane in a zeroed
 * frame of max(64, max_cells) + max_cells + 32 cells (rounded up to 8), and the pooled plane, de-interleaved by phase; about
 * 2 (width + 2 frame)(height + 2 frame) bytes.  RSX_ERR_BAD_ARG before any likelihood exists.  Asynchronous on `stream`, one launch
 * (and a memset of the two buffers when it allocates them). */
int rsx_gridmap_search_prepare(rsx_gridmap *h, int32_t max_cells, void *stream);
/* n_jobs jobs against the prepared snapshot.  Host buffers, synchronous.  out_bounds (may be NULL): uint32 [job][2K + 1][nbv][nbu].
 * The offsets are checked, a job above the cap refuses the batch; before any prepare, or with U or V above the prepared max_cells,
 * the call is RSX_ERR_BAD_ARG and touches nothing.  Staged in sub-batches of at most 64 MB of bounds (a job's bytes do not depend
 * on the cut). */
int rsx_gridmap_search_batch(rsx_gridmap *h, const float *xy, const int64_t *offsets, int32_t n_jobs, const double *priors,
                             const rsx_gridmap_search_params *params, rsx_gridmap_search_result *out_results, uint32_t *out_bounds);
/* device buffers, asynchronous on `stream`: three launches, no host synchronisation; point_stride >= 2 as for
 * rsx_gridmap_match_batch_device; the offsets are trusted; a job above the cap gets RSX_GRIDMAP_MATCH_STATUS_POINTS.
 * n_jobs (2K + 1) < 2^31.  Workspace: 16 bytes per (job, k) and 4 per job, and with d_bounds NULL the bounds, n_jobs (2K + 1) nbv nbu * 4 bytes,
 * in buffers of the handle that grow (to the next power of two) and are never given back before destroy. */
int rsx_gridmap_search_batch_device(rsx_gridmap *h, const float *d_xy, const int64_t *d_offsets, int32_t point_stride, int32_t n_jobs,
                                    const double *d_priors, const rsx_gridmap_search_params *params, rsx_gridmap_search_result *d_results,
                                    uint32_t *d_bounds, void *stream);

/* ---- the pose below the cell (csrc/gridrefine.hip): rsx_gridmap_match_* and rsx_gridmap_search_* stop at the grid, a whole-cell shift
 * and a whole rotation step.  This refines such a pose on the bilinearly interpolated likelihood plane: Gauss-Newton with
 * Levenberg-Marquardt damping and an accept test (Hector SLAM's matcher; the stage that Olson's and Cartographer's matchers put
 * behind the correlative one).  None of this is in the reference checkout: the rule below is restated in tests/gridrefine_np.py,
 * which is the arithmetic contract -- parity unpinned; the records equal the restatement's byte for byte.
 * A job is rsx_gridmap_match_*'s: the points [offsets[i], offsets[i + 1]) of a float x, y array, at most
 * RSX_GRIDMAP_MATCH_MAX_POINTS, and a prior of six doubles r00 r01 tx r10 r11 ty -- typically the transform of a match or search
 * record.  The plane L is the handle's likelihood plane, uint8, cells outside the map reading 0.  All arithmetic is fp64 on plain
 * operations, nothing fused.
 * ONE EVALUATION at a pose (r00 r01 tx r10 r11 ty).  A point with a non-finite x or y is skipped entirely.  Every other point (x, y):
 *   1. rx = r00 x + r01 y, ry = r10 x + r11 y
 *   2. fx = ((rx + tx) - origin_x) inv_res, fy = ((ry + ty) - origin_y) inv_res, inv_res = 1.0 / resolution made on the host
 *   3. the point is PLACED iff fx >= -64 && fx < width + 64 && fy >= -64 && fy < height + 64 (step 4 of the matching rule)
 *   4. a finite point that is not placed contributes r = 255, M = 0 and a zero Jacobian (gx = gy = jt = 0): what it would read deep in
 *      the zero frame, so that the cost stays comparable between poses
 *   5. placed: samples sit at cell centres: px = fx - 0.5, py = fy - 0.5, i0 = floor(px), j0 = floor(py), a = px - i0, b = py - j0
 *   6. l00 = L[j0][i0], l01 = L[j0][i0 + 1], l10 = L[j0 + 1][i0], l11 = L[j0 + 1][i0 + 1], as doubles
 *   7. top = (1 - a) l00 + a l01, bot = (1 - a) l10 + a l11, M = (1 - b) top + b bot
 *   8. gx = (1 - b)(l01 - l00) + b (l11 - l10), gy = (1 - a)(l10 - l00) + a (l11 - l01)
 *   9. jt = (gy rx - gx ry) inv_res: the rotation is about the sensor's position, in the map frame
 *  10. r = 255 - M
 * The eleven sums: cost = sum r r; score = sum M; g = sum (gx r, gy r, jt r); H = sum (gx gx, gx gy, gx jt, gy gy, gy jt, jt jt).
 * ORDER of every sum (part of the contract): partial p[t], t = 0 .. 255, is the sequential sum over points t, t + 256, ... of the
 * job in that order, starting from 0.0; the total is the balanced adjacent tree over the 256 partials, a[i] = a[2 i] + a[2 i + 1]
 * eight times.
 * THE LOOP.  Evaluate at the prior: cost_initial, score_initial.  lambda = damping.  While evaluations < max_evaluations:
 *   1. a_ii = H_ii (1 + lambda); the off-diagonals stay H's
 *   2. solve a delta = g by LDL^T written out, no square root:
 *        d0 = a00; l10 = a01 / d0; l20 = a02 / d0; d1 = a11 - l10 a01; e = a12 - l20 a01; l21 = e / d1; d2 = (a22 - l20 a02) - l21 e;
 *      each pivot must be > 0 as it is formed (a NaN fails): otherwise status SINGULAR, stop;
 *        z0 = g0; z1 = g1 - l10 z0; z2 = (g2 - l20 z0) - l21 z1; w_i = z_i / d_i;
 *        delta2 = w2; delta1 = w1 - l21 delta2; delta0 = (w0 - l10 delta1) - l20 delta2
 *   3. clamp delta0 and delta1 to +- max_shift_step (cells), delta2 to +- max_rotation_step, each by two comparisons (v > m ? m : v,
 *      then v < -m ? -m : v: a NaN passes through, its trial is rejected)
 *   4. the trial pose: tx' = tx + delta0 resolution, ty' = ty + delta1 resolution; (cs, sn) = the fixed polynomials of the deskewing
 *      model (csrc/mocomp_dev.h) at delta2; r00' = cs r00 - sn r10, r01' = cs r01 - sn r11, r10' = sn r00 + cs r10, r11' = sn r01 + cs r11
 *   5. evaluate at the trial pose
 *   6. cost' < cost: ACCEPT -- pose, sums and counts become the trial's, accepted += 1, lambda = max(lambda / 10, 1e-9); stop as
 *      converged if max(|delta0|, |delta1|) < shift_tolerance && |delta2| < rotation_tolerance
 *   7. otherwise lambda = 10 lambda; stop as converged if lambda > 1e6: nothing better is within reach
 * When the budget runs out first the status is MAX.  The returned pose is the last accepted one, so cost <= cost_initial always;
 * with nothing accepted the returned transform is the prior, bit for bit.
 * Status: RSX_GRIDMAP_MATCH_STATUS_TRANSFORM, a non-finite prior: the job is skipped, its record zero but for the status.  _POINTS
 * (device entry only; the host entry refuses the batch): more than the cap of points, treated like _TRANSFORM.  _EMPTY:
 * score_initial == 0: one evaluation, the prior is returned.  RSX_GRIDMAP_REFINE_STATUS_SINGULAR, _MAX: as above.  0: converged.
 * The Hessian's units are likelihood (the plane's byte) per cell (x, y) and per radian, multiplied in pairs: it is the curvature of
 * the cost at the returned pose, which a pose graph would weigh the constraint by.  It is NOT a calibrated covariance.
 * One launch per call whatever the batch: one workgroup of 256 threads per job runs the whole iteration; no atomics, no host round
 * trip.  Throughput comes from the jobs of a batch. */

#define RSX_GRIDMAP_REFINE_STATUS_SINGULAR 16
#define RSX_GRIDMAP_REFINE_STATUS_MAX 32

typedef struct {
  double damping;            /* the first lambda; > 0 and finite (1e-3) */
  double max_shift_step;     /* [cells] a step's |delta0|, |delta1| at the most; in (0, 8] (1.0) */
  double max_rotation_step;  /* [rad] a step's |delta2| at the most; in (0, 0.5], the polynomials' range (0.02) */
  double shift_tolerance;    /* [cells] >= 0 and finite (1e-3) */
  double rotation_tolerance; /* [rad] >= 0 and finite (1e-5) */
  int32_t max_evaluations;   /* 1 .. 64 (32) */
  int32_t reserved;          /* 0 */
} rsx_gridmap_refine_params; /* 48 bytes */

typedef struct {
  double transform[6];       /* r00 r01 tx r10 r11 ty: the returned pose */
  double hessian[6];         /* H00 H01 H02 H11 H12 H22, undamped, at the returned pose */
  double cost_initial, cost; /* sum r r at the prior and at the returned pose */
  double score_initial, score; /* sum M at the prior and at the returned pose */
  int32_t evaluations, accepted;
  int32_t n_points;          /* points placed at the returned pose */
  int32_t n_inside;          /* of those, floor(fx), floor(fy) inside the map */
  int32_t status;            /* RSX_GRIDMAP_MATCH_STATUS_* | RSX_GRIDMAP_REFINE_STATUS_* */
  int32_t reserved;          /* 0 */
} rsx_gridmap_refine_result; /* 152 bytes */

/* a violated rule of rsx_gridmap_refine_params gives RSX_ERR_BAD_ARG in every entry that takes the struct (NULL = the defaults),
 * judged before the handle or the device is looked at */
int rsx_gridmap_refine_default_params(rsx_gridmap_refine_params *p);
/* n_jobs jobs against the likelihood plane.  Host buffers, synchronous.  The offsets are checked, a job above the cap refuses the
 * batch; before any likelihood exists the call is RSX_ERR_BAD_ARG and touches nothing. */
int rsx_gridmap_refine_batch(rsx_gridmap *h, const float *xy, const int64_t *offsets, int32_t n_jobs, const double *priors,
                             const rsx_gridmap_refine_params *params, rsx_gridmap_refine_result *out_results);
/* device buffers, asynchronous on `stream`: one launch, no allocation, no host synchronisation; point_stride >= 2 as for
 * rsx_gridmap_match_batch_device; the offsets are trusted; a job above the cap gets RSX_GRIDMAP_MATCH_STATUS_POINTS. */
int rsx_gridmap_refine_batch_device(rsx_gridmap *h, const float *d_xy, const int64_t *d_offsets, int32_t point_stride, int32_t n_jobs,
                                    const double *d_priors, const rsx_gridmap_refine_params *params, rsx_gridmap_refine_result *d_results,
                                    void *stream);

/* ---- a likelihood field in the plane (csrc/gridfield.hip): the three localisers above read one frozen uint8 plane, and on a raw radar
 * plane (the mean, the hits) the refinement converges only from nearby.  This fills the plane with a function of the distance to the
 * map's structure instead -- the likelihood field of AMCL and Hector SLAM, Cartographer's smoothed probability grid -- by an exact
 * Euclidean distance transform, truncated at a radius.  None of this is in the reference checkout: the rule below is restated in
 * tests/gridfield_np.py, which is the arithmetic contract -- parity unpinned.  Integers throughout: the plane equals the restatement's
 * byte for byte, every cell.
 * rsx_gridmap_likelihood_field transforms the likelihood plane of the handle IN PLACE, whatever filled it (the mean, the hits, a loaded
 * image, a field):
 *   1. a map cell is a SEED iff its byte >= threshold; the cells of the frame are never seeds
 *   2. q(x, y) = the smallest dx dx + dy dy over the seeds (x + dx, y + dy) with dx dx + dy dy <= radius radius: an integer, exact
 *   3. the new byte is table[q], and 0 where no seed lies within the radius; table: the caller's uint8 [radius radius + 1]
 *   4. the frame of 128 cells stays zero
 * A second call transforms the field itself (its seeds: the field's bytes >= threshold); that is defined and nothing special.
 * The device evaluates no exponential: the table is an input, so that the bytes cannot hinge on a libm's last bit.
 * rsx_gridmap_field_gaussian_table makes the usual one on the host, in fp64: out[q] = (uint8)floor(peak exp(-q / (2 sigma sigma)) + 0.5),
 * q = 0 .. radius radius, the exponent formed as -(double)q / ((2.0 * sigma) * sigma).
 * The field costs accuracy (its seeds are whole cells), so the chain is: refine on the field from far away, then update the plane from
 * the mean and refine again (tests/test_gridfield_restatement.py has the figures of both stages on the synthetic drive).
 * rsx_gridmap_search_prepare snapshots the plane: a search in the field needs a prepare AFTER this call.
 * Two launches per call whatever the map: the seeds as a bit per cell (one 64-bit ballot per wavefront); then one workgroup per tile
 * of 64 x 32 cells, which reads bits only, never a byte that another workgroup writes: the bit rows of the tile and a halo of `radius`
 * go into LDS, the distance to the nearest seed along its own row comes from a count of leading / trailing zeros on the windowed
 * words, q is the smallest dy dy + that distance squared over |dy| <= radius, and the table sits in LDS too.  No atomics. */

typedef struct {
  int32_t threshold;  /* a cell is a seed iff its byte >= threshold; 1 .. 255 (50) */
  int32_t radius;     /* [cells] 1 .. 64 (12) */
  int32_t reserved0;  /* 0 */
  int32_t reserved1;  /* 0 */
} rsx_gridmap_field_params; /* 16 bytes */

#define RSX_GRIDMAP_FIELD_MAX_RADIUS 64

/* threshold 50, radius 12 (and, with table NULL below, sigma 3 cells and peak 255): the values of a prototype on the hits plane of the
 * synthetic drive (cells of 1 m).  NO REAL RADAR DATA BACKS THEM.  A violated rule of rsx_gridmap_field_params gives RSX_ERR_BAD_ARG,
 * judged before the handle or the device is looked at */
int rsx_gridmap_field_default_params(rsx_gridmap_field_params *p);
/* host only, no device: out[0 .. radius radius] by the formula above; sigma_cells > 0 and finite, peak 1 .. 255, radius 1 .. 64, else
 * RSX_ERR_BAD_ARG.  out[0] == peak and the table does not increase */
int rsx_gridmap_field_gaussian_table(double sigma_cells, int32_t peak, int32_t radius, uint8_t *out);
/* the transform.  params NULL: the defaults; table (host memory, radius radius + 1 bytes) NULL: the Gaussian of sigma 3, peak 255 at
 * the radius of params.  RSX_ERR_BAD_ARG before any likelihood exists (nothing is allocated then).  Asynchronous on `stream`, two
 * launches, ordered like rsx_gridmap_likelihood_update; the caller may free table on return: the handle keeps a copy on the host and on
 * the device, and a call whose table differs from the previous call's uploads it and waits for that one copy (4097 bytes at the most)
 * before it launches.  Workspace, allocated at the first call and kept until destroy: width height / 8 bytes of seeds and the table. */
int rsx_gridmap_likelihood_field(rsx_gridmap *h, const rsx_gridmap_field_params *params, const uint8_t *table, void *stream);

/* ---- following a sensor through the map, scan after scan (csrc/gridtrack.hip): match on the grid around a constant-velocity
 * prediction, refine below the cell, compose the motion -- whole sequences in ONE launch, one workgroup per sequence, the state
 * resident in device memory (what rsx_cfear_tracker_* is to rsx_cfear_register_*).  None of this is in the reference checkout: the
 * rule below is restated in tests/gridtrack_np.py, which is the arithmetic contract -- parity unpinned; the records equal the
 * restatement's byte for byte.
 * All arithmetic of the glue is fp64 on plain operations, nothing fused, every expression formed in the order written; no square root,
 * sine or cosine.  Poses are six doubles r00 r01 tx r10 r11 ty (indices 0 .. 5):
 *   mul(A, B)  = (A0 B0 + A1 B3,  A0 B1 + A1 B4,  (A0 B2 + A1 B5) + A2,
 *                 A3 B0 + A4 B3,  A3 B1 + A4 B4,  (A3 B2 + A4 B5) + A5)
 *   inv(A)     = (A0, A3, -(A0 A2 + A3 A5),  A1, A4, -(A1 A2 + A4 A5))
 *   renorm(T)  : n2 = T0 T0 + T3 T3;  f = 1.5 - 0.5 n2;  c = T0 f;  s = T3 f;   -> (c, -s, T2, s, c, T5)
 * renorm is one Newton step towards a unit first column and rebuilds the second from it.  It is part of the rule: match turns its
 * prior by fp32-rounded (c, s), and the chain inv, mul compounds that -- without it det R is 1 + 6.6e-5 after 10 scans of the synthetic
 * drive and growing; with it |det R - 1| <= 2e-15 after 16.
 * State per sequence: the pose P, the motion M (the identity after a reset) and n, the scans seen since the reset.  Per scan, cloud xy:
 *   1. start = P when n == 0 or predict == 0, else renorm(mul(P, M)): scan 0 is matched from the reset pose bit for bit
 *   2. m = the record of the rule of rsx_gridmap_match_* for (xy, prior start, params.match)
 *   3. the scan is LOST iff m.status != 0 or m.score < min_score (the device entry's _POINTS counts as m.status != 0).  Then
 *      P = start, M stays, the refine record is all zero, flags = RSX_GRIDMAP_TRACK_LOST
 *   4. otherwise r = the record of the rule of rsx_gridmap_refine_* for (xy, prior m.transform, params.refine); every refine status is
 *      accepted, because its cost never rises.  new = renorm(r.transform); if n > 0, M = mul(inv(P), new); P = new; flags = 0
 *   5. n += 1; the record's transform is P after the scan
 * A lost scan dead-reckons; re-localising it is the caller's job: rsx_gridmap_search_*, then rsx_gridmap_tracker_set_pose.
 * The tracker reads the map's likelihood plane as it stands at each push and locks the map's mutex; its calls are ordered with the
 * map's own (rsx_gridmap_likelihood_*, ...) through the map's stream order.  The map must outlive the tracker.
 * One launch per push whatever the batch: one workgroup of 256 threads per sequence loops over the sequence's scans of the push; per
 * rotation the cloud's cells go into LDS and the slot sums of the match kernel run, the score volume ((2K + 1)(2V + 1)(2U + 1) <= 4913
 * words) never leaves LDS, the pick and the refinement loop are the device functions that rsx_gridmap_match_* and rsx_gridmap_refine_*
 * run.  No atomics on device memory, no dependence between workgroups.  Throughput comes from sequences side by side. */

#define RSX_GRIDMAP_TRACK_LOST 1
#define RSX_GRIDMAP_TRACK_MAX_ANGLE_STEPS 8
#define RSX_GRIDMAP_TRACK_MAX_CELLS 8

typedef struct {
  rsx_gridmap_match_params match;    /* K <= 8, U, V <= 8 here (defaults 2, 2, 2, angle_step 0.01) */
  rsx_gridmap_refine_params refine;  /* its own rules and defaults */
  uint32_t min_score;                /* 0 = none (0): no real radar data backs any other value */
  int32_t predict;                   /* 0 / 1 (1) */
  int32_t reserved[2];               /* 0 */
} rsx_gridmap_track_params;          /* 88 bytes */

typedef struct {
  double transform[6];               /* P after the scan */
  double start[6];                   /* the prior the scan was matched from */
  rsx_gridmap_match_result match;    /* 88 bytes */
  rsx_gridmap_refine_result refine;  /* 152 bytes; all zero on a lost scan */
  int32_t flags;                     /* RSX_GRIDMAP_TRACK_* */
  int32_t reserved;                  /* 0 */
} rsx_gridmap_track_result;          /* 344 bytes */

typedef struct rsx_gridmap_tracker rsx_gridmap_tracker;

/* a violated rule of rsx_gridmap_track_params (its match and refine parts included) gives RSX_ERR_BAD_ARG in both pushes (NULL = the
 * defaults), judged before the handle or the device is looked at */
int rsx_gridmap_track_default_params(rsx_gridmap_track_params *p);
/* n_sequences (1 .. 4096) sequences in `map`, every one at the identity pose with n = 0.  104 bytes of state per sequence */
int rsx_gridmap_tracker_create(rsx_gridmap *map, int32_t n_sequences, rsx_gridmap_tracker **out);
int rsx_gridmap_tracker_destroy(rsx_gridmap_tracker *h);
/* poses: host, [n_sequences][6].  Every sequence: P = its pose, M = the identity, n = 0.  A non-finite entry gives RSX_ERR_BAD_ARG and
 * changes nothing.  Synchronous. */
int rsx_gridmap_tracker_reset(rsx_gridmap_tracker *h, const double *poses);
/* one sequence (0 .. n_sequences - 1): P = pose6 (finite), M = the identity, n = 0.  Synchronous. */
int rsx_gridmap_tracker_set_pose(rsx_gridmap_tracker *h, int32_t sequence, const double *pose6);
/* the state to host arrays [n_sequences][6], [n_sequences][6], [n_sequences]; any pointer may be NULL.  Synchronous. */
int rsx_gridmap_tracker_state(rsx_gridmap_tracker *h, double *out_poses, double *out_motions, int32_t *out_counts);
/* n_scans[q] >= 0 scans for sequence q, sequence after sequence (rsx_cfear_tracker_push's layout): scan j of the total owns the points
 * [offsets[j], offsets[j + 1]) of xy and out[j].  Host buffers, synchronous.  The offsets are checked; a scan above
 * RSX_GRIDMAP_MATCH_MAX_POINTS refuses the batch.  Before any likelihood exists on the map the call is RSX_ERR_BAD_ARG and touches
 * nothing.  The parameters may differ from push to push (the state holds none); the records do not depend on how a sequence is cut
 * into pushes, on how many sequences run side by side, or on a sequence's index. */
int rsx_gridmap_tracker_push(rsx_gridmap_tracker *h, const float *xy, const int64_t *offsets, const int32_t *n_scans,
                             const rsx_gridmap_track_params *params, rsx_gridmap_track_result *out);
/* device buffers, asynchronous on `stream`: one launch, no allocation, no host synchronisation.  point_stride >= 2 as for
 * rsx_gridmap_match_batch_device; d_n_scans: int32 [n_sequences] in device memory; total_scans: the records that d_out and the
 * offsets (total_scans + 1) have room for -- a scan whose index is total_scans or more is neither read nor written nor counted.  The
 * offsets are trusted; a scan above the cap is LOST with RSX_GRIDMAP_MATCH_STATUS_POINTS. */
int rsx_gridmap_tracker_push_device(rsx_gridmap_tracker *h, const float *d_xy, const int64_t *d_offsets, int32_t point_stride,
                                    const int32_t *d_n_scans, int32_t total_scans, const rsx_gridmap_track_params *params,
                                    rsx_gridmap_track_result *d_out, void *stream);

/* ============================== ORORA front end ========================================
 * The steps between the cen2019 keypoints and the solver in the upstream file-based entry (reference README.md:26-29;
 * SURVEY 8f rank 3): polar -> Cartesian image, ORB-style binary descriptors at the keypoints, brute-force Hamming
 * knnMatch(k = 2) + ratio test.  Upstream uses OpenCV for all three; the sources are absent from the reference checkout,
 * so these follow the published steps as restated in oracle/frontend_ref.c -- parity unpinned (in particular the 256
 * test pairs come from a seeded generator, not OpenCV's learned table: not byte-compatible with cv::ORB). */

typedef struct rsx_frontend rsx_frontend;

typedef struct {
  int32_t cart_pixel_width; /* W: the Cartesian image is W x W, centred on the sensor (964) */
  float cart_resolution;    /* metres per pixel (0.2592) */
  float ratio;              /* default nearest-neighbour distance ratio of rsx_frontend_match callers (0.8) */
  int32_t flags;            /* RSX_FRONTEND_*; 0 = default */
} rsx_frontend_params;
#define RSX_FRONTEND_THREE_PASS 1     /* remap, blur rows, blur columns as three kernels instead of the one strip kernel (same images) */
#define RSX_FRONTEND_EXACT_AZIMUTH 2  /* decide every pixel's azimuth row by the fp64 division (default: a reciprocal multiply with a proven \
                                         margin, the division only where the margin does not decide; same images) */
#define RSX_FRONTEND_TILES 4          /* the 32 x 32 LDS-tile kernel of round 3 instead of the strip kernel (same images) */

int rsx_frontend_default_params(rsx_frontend_params *p);
/* one handle per polar image shape (rows azimuths x cols range bins) */
int rsx_frontend_create(int device, int32_t rows, int32_t cols, const rsx_frontend_params *params, rsx_frontend **out);
int rsx_frontend_destroy(rsx_frontend *h);
/* polar image (host bytes, same layout arguments as rsx_cen2019_extract; azimuths = rows floats in rad, increasing)
 * -> Cartesian fp32 image, kept on the GPU together with its 7 x 7 Gaussian-smoothed copy for rsx_frontend_describe;
 * out_cart (optional, W * W floats, row 0 = farthest forward, forward = azimuth 0, azimuth grows to the right) */
int rsx_frontend_cartesian(rsx_frontend *h, const uint8_t *img, int32_t row_stride, int32_t col_offset, const float *azimuths,
                           float resolution, float *out_cart);
/* 256-bit descriptors of n keypoints given in metres in the sensor frame (x forward, y right: the out_xy of
 * rsx_cen2019_extract) on the last image: out_desc n x 32 bytes, out_valid[i] = 0 when the patch leaves the image */
int rsx_frontend_describe(rsx_frontend *h, const float *xy, int32_t n, uint8_t *out_desc, uint8_t *out_valid);
/* knnMatch(k = 2) + ratio test of nq query descriptors against nt train descriptors: out_train_idx[i] = the nearest
 * train descriptor if d1 < ratio * d2, else -1; out_d1 / out_d2 (optional) the two smallest Hamming distances (-1: none) */
int rsx_frontend_match(rsx_frontend *h, const uint8_t *q_desc, const uint8_t *q_valid, int32_t nq, const uint8_t *t_desc,
                       const uint8_t *t_valid, int32_t nt, float ratio, int32_t *out_train_idx, int32_t *out_d1, int32_t *out_d2);

/* the batched / device-resident forms of the three calls above (what rsx_odometry chains; usable on their own):
 * Cartesian images + smoothed copies of n_images scans resident in HBM, kept in the handle's slots 0 .. n_images-1
 * (azimuths: HOST array, rows floats, ONE grid used for every image of the batch; per-image grids: the _az form below) */
int rsx_frontend_cartesian_batch_device(rsx_frontend *h, const uint8_t *d_imgs, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride,
                                        int32_t col_offset, const float *azimuths, float resolution, void *stream);
/* the same with the azimuth grids in DEVICE memory, one per image: image i samples the grid at d_azimuths + i *
 * azimuth_stride_floats (its first two entries give start and step; 0: one grid for every image).  MulRan scans carry their
 * own encoder grid; a map built from the first scan's grid would rotate every other scan's Cartesian image against its own
 * keypoints.  Nothing is read on the host: no synchronisation, whatever the grids do from window to window. */
int rsx_frontend_cartesian_batch_device_az(rsx_frontend *h, const uint8_t *d_imgs, int32_t n_images, int64_t image_stride_bytes,
                                           int32_t row_stride, int32_t col_offset, const float *d_azimuths, int64_t azimuth_stride_floats,
                                           float resolution, void *stream);
/* descriptors of the keypoints of every image of that batch: d_xy [n_images][max_targets][2] and d_counts [n_images] as
 * rsx_cen2019_extract_batch_device leaves them -> d_desc [n_images][max_targets][32], d_valid [n_images][max_targets] */
int rsx_frontend_describe_batch_device(rsx_frontend *h, const float *d_xy, const int32_t *d_counts, int32_t n_images, int32_t max_targets,
                                       uint8_t *d_desc, uint8_t *d_valid, void *stream);
/* knnMatch(2) + ratio between CONSECUTIVE keypoint sets of [slot][max_targets] arrays: pair j = (slot first_slot + j,
 * slot first_slot + j + 1); d_fwd [n_pairs][max_targets]: for every keypoint of the first slot its match in the second
 * (or -1), d_bwd the reverse direction */
int rsx_frontend_match_consecutive_device(rsx_frontend *h, const uint8_t *d_desc, const uint8_t *d_valid, const int32_t *d_counts,
                                          int32_t max_targets, int32_t first_slot, int32_t n_pairs, float ratio, int32_t *d_fwd,
                                          int32_t *d_bwd, void *stream);

/* ============================== file-based odometry pipeline ============================
 * The main loop of the upstream file-based `odometry.cpp` entry (reference README.md:26-29,54-60; launched through
 * $(find orora)/launch/run_orora.launch, launch/navtech_radar_slam_mulran.launch:5-8): polar scan -> cen2019 keypoints ->
 * Cartesian image + ORB-style descriptors -> knnMatch(2) + ratio + cross check against the previous scan -> ORORA.
 * The sequence is on disk, so a caller hands over WINDOWS of consecutive scans: every stage runs once per window for all
 * scans / all consecutive pairs, everything between the image upload and the 48-byte result per scan stays in HBM, and
 * ORORA registers all pairs of a window in one batch.  The handle remembers the last scan (on the device), so the pair
 * that straddles two calls is registered too.  Pose composition (sequential, trivial) is the caller's.  Sources of the
 * upstream entry are absent from the reference checkout (empty submodule) -- parity unpinned. */

typedef struct rsx_odometry rsx_odometry;

typedef struct {
  rsx_cen2019_params cen;
  rsx_frontend_params frontend;  /* frontend.ratio = the knnMatch ratio */
  rsx_orora_params orora;
  float radar_resolution;        /* metres per range bin (0.0595: Navtech CIR204-H / MulRan) */
  int32_t col_offset;            /* metadata bytes in front of the power samples of every row (11) */
  int32_t max_keypoints;         /* keypoints kept per scan (16384 = rsx_orora_max_correspondences(), its upper limit) */
  int32_t device;
} rsx_odometry_params;

typedef struct {
  rsx_orora_result reg;  /* motion between the previous scan and this one: p_previous = R(yaw) p_this + (x, y);
                            reg.status = 3 for the first scan of a sequence (nothing to register against) */
  int32_t n_keypoints;   /* keypoints of this scan (cen2019, or cen2018 / k-strongest / CFAR: rsx_odometry_set_cen2018 / _set_kstrongest / _set_cfar; only the first max_keypoints are used) */
  int32_t n_matches;     /* cross-checked ratio matches handed to ORORA */
} rsx_odometry_scan;

int rsx_odometry_default_params(rsx_odometry_params *p);
/* (device memory of a handle for 400 x 3360 scans: about 4 GB -- two extraction lanes of a 64-scan window each, three sets of
 * keypoints / descriptors, allocated at the first push; three windows of a sequence are in flight inside a call) */
int rsx_odometry_create(const rsx_odometry_params *params, int32_t rows, int32_t cols, rsx_odometry **out);
int rsx_odometry_destroy(rsx_odometry *h);
int rsx_odometry_reset(rsx_odometry *h); /* forget the previous scan: the next scan starts a new sequence */
int rsx_odometry_window(void);           /* scans per internal launch chain (longer calls are cut into such windows) */
/* keypoints by cen2018 with these settings instead of cen2019 (params = NULL: back to cen2019, the default).  Only while
 * the handle holds no scan -- freshly created or after rsx_odometry_reset -- so that no pair is registered from keypoints of
 * two extractors; otherwise RSX_ERR_BAD_ARG.  rsx_odometry_scan.n_keypoints then counts cen2018 keypoints. */
int rsx_odometry_set_cen2018(rsx_odometry *h, const rsx_cen2018_params *params);
/* keypoints by k-strongest with these settings (rsx_kstrongest above).  Either setter selects its extractor in place of
 * whichever was selected, and params = NULL in either goes back to cen2019.  The same rule: only while the handle holds no
 * scan.  Independent of estimator and compensation.  At most rows x k keypoints per scan, of which the first max_keypoints
 * are used. */
int rsx_odometry_set_kstrongest(rsx_odometry *h, const rsx_kstrongest_params *params);
/* keypoints by CA-CFAR / BFAR with these settings (rsx_cfar above), under the rules of the two setters above: accepted only
 * while the handle holds no scan, params = NULL goes back to cen2019, independent of estimator, compensation and the CFEAR
 * switches.  At most rows x k keypoints per scan, of which the first max_keypoints are used. */
int rsx_odometry_set_cfar(rsx_odometry *h, const rsx_cfar_params *params);
/* The motion estimator a pair's cross-checked matches go to: ORORA behind the max-clique selection (the default), rigid
 * RANSAC or motion-compensated RANSAC (params = NULL: rsx_ransac_default_params; its MOTION_COMPENSATED flag follows
 * `estimator`).  Independent of the extractor; like it, only accepted while the handle holds no scan.  With a RANSAC
 * estimator the max-clique selection (an ORORA stage) does not run and rsx_odometry_scan.reg carries x, y, yaw and status
 * (0, 1, 2 as for ORORA; 4: no hypothesis had 2 inliers), iterations = hypotheses evaluated, rot_inliers = trans_inliers =
 * inliers.  MC time model: the keypoint on azimuth row a of a scan was measured (a + 0.5) / rows x dt_scan after the
 * scan's start and scans start dt_scan apart, so a match of row a_cur of this scan with row a_prev of the previous one
 * has dt = (float)(dt_scan x (1 + (a_cur - a_prev) / rows)); the pose is exp(dt_scan w), so the body velocity is
 * log(pose) / dt_scan.  Per-row timestamps from the image metadata and dropped scans are not modelled. */
#define RSX_ESTIMATOR_ORORA 0
#define RSX_ESTIMATOR_RANSAC 1
#define RSX_ESTIMATOR_MCRANSAC 2
int rsx_odometry_set_estimator(rsx_odometry *h, int estimator, const rsx_ransac_params *params);
/* Motion and Doppler compensation of the keypoints (rsx_mocomp above; params->flags picks the corrections, params->rows is
 * ignored: the handle's rows count).  NULL switches it off, which is the default.  Accepted only while the handle holds no
 * scan, with RSX_ESTIMATOR_ORORA and RSX_ESTIMATOR_RANSAC; RSX_ERR_BAD_ARG with RSX_ESTIMATOR_MCRANSAC, which has its own
 * motion model (and rsx_odometry_set_estimator refuses MC-RANSAC while compensation is on).  With it a pair is estimated,
 * compensated with its own estimate and estimated again, all pairs of a window in one batch each time: pass 1 as without
 * compensation; the matches of every pair are then compensated with the velocity log(pose) / dt_scan of the pose pass 1 gave
 * that pair; the same estimator (max-clique selection and solver, or RANSAC) runs once more on the compensated matches, and
 * rsx_odometry_scan.reg is that second result.  A pair whose first pass has status != 0 is not compensated and keeps its
 * first result; so does, in effect, a pair with |yaw| > 0.5 (RSX_MOCOMP_STATUS_ANGLE: its matches stay as measured).  One
 * round only.  out_xy carries scan i's keypoints compensated with the velocity of the pair (i-1, i) (the second result;
 * uncompensated when that pair's status != 0 and for the first scan of a sequence); what is matched and carried to the next
 * window stays uncompensated.  Results do not depend on how the sequence is cut into calls. */
int rsx_odometry_set_compensation(rsx_odometry *h, const rsx_mocomp_params *params);
/* CFEAR's own pipeline (rsx_cfear above) in place of the descriptors, the matcher and the estimator: after the keypoint
 * extractor the surface points of every scan are built, and the consecutive pairs of a window are registered point-to-line,
 * src = this scan, dst = the previous one, identity start.  The Cartesian image, the descriptors, the matcher, the cross
 * check and the max-clique selection do not run.  params = NULL goes back to ORORA.  Accepted only while the handle holds no
 * scan; RSX_ERR_BAD_ARG while compensation is on (and rsx_odometry_set_compensation refuses while CFEAR is selected: the
 * MC-RANSAC rule).  rsx_odometry_set_estimator leaves CFEAR as it leaves any other estimator, but refuses RSX_ESTIMATOR_CFEAR
 * itself: this setter carries the parameters.  Independent of the extractor; the documented pairing is k-strongest with
 * min_separation = 0.  rsx_odometry_scan.reg carries x, y, yaw and status of the rsx_cfear_result, iterations = its
 * iterations, rot_inliers = trans_inliers = n_matches = its correspondences.  A scan with more than
 * RSX_CFEAR_MAX_SURFACE_POINTS surface points gives its pairs status 2.  Results do not depend on how the sequence is cut
 * into calls. */
#define RSX_ESTIMATOR_CFEAR 3
int rsx_odometry_set_cfear(rsx_odometry *h, const rsx_cfear_params *params);
/* CFEAR's keyframe tracker (rsx_cfear_tracker above) in place of the registration of consecutive pairs: in a window ONE tracker
 * launch over the window's scans replaces the registration launch; its state (pose, motion, ring of keyframes) lives in the handle
 * and starts again with every new sequence (rsx_odometry_reset).  Accepted only while CFEAR is selected and the handle holds no
 * scan; params = NULL goes back to pairs (as does leaving CFEAR); without this call nothing changes.  rsx_odometry_scan.reg carries
 * the relative motion P_{i-1}^-1 o P_i of the tracked poses, with status, iterations and correspondences of the scan's registration
 * against its keyframes as above (status 1, 2, 4, 5: the motion is the prediction's); the first scan's status stays 3.  Results do
 * not depend on how the sequence is cut into calls.
 * params->compensate = 1: the window builds the surface points with their times (rsx_cfear_surface_points_timed_batch: the rows of
 * the extractor's targets, n_rows = the image's rows, at most 65536) and runs the tracker's two-pass rule on them
 * (rsx_cfear_tracker_push_timed).  out_xy stays the keypoints as measured: what compensation would mean for the published cloud
 * is out of scope.  rsx_odometry_set_compensation, which compensates MATCHES, still refuses while CFEAR is selected. */
int rsx_odometry_set_cfear_tracking(rsx_odometry *h, const rsx_cfear_track_params *params);
/* Phase correlation (rsx_phasecorr above) in the window pipeline, in one of two modes.  Accepted only while the handle holds no scan;
 * params = NULL switches it off (the selected estimator, which ESTIMATE stands in for but never replaces, alone).  pc is judged by
 * the rules of rsx_phasecorr_params against the handle's rows and cols (RSX_ERR_BAD_ARG), after pc.range_resolution has been
 * overwritten with (double)radar_resolution of the handle; negative or non-finite gates and an unknown mode are refused too.  Refused
 * while compensation is on and while the CFEAR tracker is on (both modes), and rsx_odometry_set_compensation and
 * rsx_odometry_set_cfear_tracking refuse in return while either mode is on.  Without this call a handle allocates and launches
 * nothing new.
 *   RSX_ODOMETRY_PHASECORR_ESTIMATE  in place of the descriptors, the matcher and the estimator.  E(g) still runs the selected
 *     keypoint extractor (n_keypoints and out_xy stay what they are) and then the spectra of the window's scans (launches 1 - 3 of
 *     rsx_phasecorr) into the set's slots 1 .. n; the last scan's spectra are carried into slot 0 of the next set
 *     (12 N^2 - 32 N bytes).  No Cartesian image, descriptors, matcher, cross check or max-clique selection run.  M(g) registers the
 *     consecutive pairs (launches 4 - 9; src = this scan, dst = the previous one) and writes the records; n_matches = 0.
 *     rsx_odometry_set_estimator and rsx_odometry_set_cfear leave this mode as they leave any other estimator, but
 *     rsx_odometry_set_estimator refuses RSX_ESTIMATOR_PHASECORR itself: this setter carries the parameters.
 *   RSX_ODOMETRY_PHASECORR_FALLBACK  beside the selected estimator (ORORA, RANSAC, MC-RANSAC or CFEAR pairs), whose whole chain runs
 *     unchanged; E(g) additionally makes and carries the spectra.  Behind the estimator M(g) lists the pairs it FAILED on -- status
 *     != 0, except CFEAR's 8 (max_iterations reached: the pose is carried) --, registers exactly those (the others take the
 *     RSX_PHASECORR_STATUS_INDEX path, on which nothing is computed) and puts the phase-correlation record in place of each failed
 *     pair's record; n_matches keeps the matcher's count.  Records of pairs that did not fail are byte for byte those of the same
 *     handle without the fallback.
 * A phase-correlation record in rsx_odometry_scan.reg (both modes): x, y, yaw = the rsx_phasecorr_result's x, y, theta, bit for bit
 * (p_previous = R(yaw) p_this + (x, y)); iterations = -1 - half_turn (negative: "this record is phase correlation's");
 * rot_inliers = (int32)rint(peak x 1e6), trans_inliers = (int32)rint(peak_ratio x 1e6); status = 0, or
 * RSX_ODOMETRY_STATUS_PHASECORR | 1 (|theta| > pc.max_rotation) | 2 (a gate failed: peak_ratio > max_peak_ratio or peak < min_peak).
 * The pose is reported as found in every case; a caller that composes poses skips status != 0 as for any other estimator.  The gates
 * default to off: the levels of peak and peak_ratio depend on N, the resolution and the scene, and none has been measured on real
 * data.  Device memory while on: per set (window + 1) x (12 N^2 - 32 N) bytes of spectra, once window x (40 N^2 + 2048 + 4 N) bytes
 * of pair workspace (N = 256: 3 x 49 MiB + 161 MiB).  Results do not depend on how the sequence is cut into calls or windows. */
#define RSX_ESTIMATOR_PHASECORR 4
#define RSX_ODOMETRY_PHASECORR_ESTIMATE 0   /* in place of descriptors, matcher and estimator */
#define RSX_ODOMETRY_PHASECORR_FALLBACK 1   /* beside the selected estimator, for the pairs it failed on */
#define RSX_ODOMETRY_STATUS_PHASECORR 16    /* base of a phase-correlation record's non-zero status */
typedef struct {
  rsx_phasecorr_params pc;   /* range_resolution is overwritten with the handle's radar_resolution */
  double max_peak_ratio;     /* gate: peak_ratio above it marks the record ambiguous; 0 = no gate (default) */
  double min_peak;           /* gate: peak below it marks the record ambiguous; 0 = no gate (default) */
  int32_t mode;              /* RSX_ODOMETRY_PHASECORR_* (ESTIMATE) */
  int32_t reserved;          /* 0 */
} rsx_odometry_phasecorr_params; /* 64 bytes */
int rsx_odometry_default_phasecorr_params(rsx_odometry_phasecorr_params *p);   /* needs no device */
int rsx_odometry_set_phasecorr(rsx_odometry *h, const rsx_odometry_phasecorr_params *params);  /* NULL: off */
/* n_scans consecutive scans, host images image_stride_bytes apart (rows x row_stride bytes each); azimuths: rows floats
 * (rad, increasing) shared by all scans or n_scans x rows when azimuths_per_image != 0.  out [n_scans]; out_xy
 * (optional) [n_scans][max_xy][2]: the scan's keypoints in metres in the sensor frame (/orora/cloud_local).  Synchronous. */
int rsx_odometry_push(rsx_odometry *h, const uint8_t *imgs, int32_t n_scans, int64_t image_stride_bytes, int32_t row_stride,
                      const float *azimuths, int32_t azimuths_per_image, rsx_odometry_scan *out, float *out_xy, int32_t max_xy);
/* the same with the images already resident in HBM (d_imgs: device pointer; everything else host) */
int rsx_odometry_push_device(rsx_odometry *h, const uint8_t *d_imgs, int32_t n_scans, int64_t image_stride_bytes, int32_t row_stride,
                             const float *azimuths, int32_t azimuths_per_image, rsx_odometry_scan *out, float *out_xy, int32_t max_xy);
/* page-locked host memory for image windows (decode threads write straight into it: the upload then runs at PCIe speed) */
int rsx_host_alloc_pinned(size_t bytes, void **out);
int rsx_host_free_pinned(void *p);

/* ============================== VoxelGrid downsample ===================================
 * pcl::VoxelGrid<pcl::PointXYZI>::filter with setLeafSize(leaf, leaf, leaf): the step right before
 * makeAndSaveScancontextAndKeys in the reference's keyframe path (PGO.cpp:98,482-484; leaf 0.4 set at
 * PGO.cpp:687-688).  PCL is not part of the reference checkout: follows the published algorithm
 * (oracle/voxelgrid_ref.c) -- parity unpinned.  Output = one centroid {x,y,z,intensity} per occupied
 * voxel, packed float4, in ascending voxel-index order.  If the voxel grid would overflow int32
 * ("leaf size too small") the input is returned unchanged, like PCL does. */

typedef struct rsx_voxelgrid rsx_voxelgrid;

int rsx_voxelgrid_create(int device, rsx_voxelgrid **out);
int rsx_voxelgrid_destroy(rsx_voxelgrid *h);
/* pts: n points stride_bytes apart, float x,y,z at byte offsets 0,4,8, float intensity at
 * intensity_offset (16 for pcl::PointXYZI; < 0: none, output 0).  Non-finite points are dropped.
 * *out_count = number of output points (only the first max_out are written). */
int rsx_voxelgrid_filter(rsx_voxelgrid *h, const void *pts, size_t n, size_t stride_bytes, int32_t intensity_offset,
                         float leaf, float *out_xyzi, int64_t max_out, int64_t *out_count);
/* downSizeFilterScancontext.filter(...) + scManager.makeAndSaveScancontextAndKeys(...) in one call
 * (PGO.cpp:482-492): the downsampled cloud never leaves the GPU.  vg and h must be on the same device. */
int rsx_sc_add_points_downsampled(rsx_sc *h, rsx_voxelgrid *vg, const void *pts, size_t n, size_t stride_bytes,
                                  float leaf, int32_t *out_index);

/* ============================== ICP loop verification ===================================
 * pcl::IterativeClosestPoint<PointXYZI, PointXYZI> as the reference configures it in
 * doICPVirtualRelative (PGO.cpp:371-392): point-to-point, SVD (Umeyama) step, PCL's default
 * convergence criteria, fitness = mean squared nearest-neighbour distance.  PCL is not part of the
 * reference checkout: follows the published algorithm (oracle/icp_ref.c) -- parity unpinned. */

typedef struct rsx_icp rsx_icp;

typedef struct {
  double max_corr_dist;             /* setMaxCorrespondenceDistance(150), PGO.cpp:374 */
  double transformation_epsilon;    /* setTransformationEpsilon(1e-6),    PGO.cpp:376 */
  double euclidean_fitness_epsilon; /* setEuclideanFitnessEpsilon(1e-6),  PGO.cpp:377 */
  int32_t max_iterations;           /* setMaximumIterations(100),         PGO.cpp:375 */
  int32_t reserved;
} rsx_icp_params;

typedef struct {
  float transform[16]; /* getFinalTransformation(): row-major 4x4, target <- source */
  double fitness;      /* getFitnessScore() */
  int32_t iterations;
  int32_t converged;   /* hasConverged() */
  int32_t state;       /* 1 iterations, 2 transform, 3 abs MSE, 4 rel MSE, 5 not enough correspondences */
  int32_t reserved;
} rsx_icp_result;

int rsx_icp_default_params(rsx_icp_params *p);
int rsx_icp_create(int device, rsx_icp **out);
int rsx_icp_destroy(rsx_icp *h);
/* icp.setInputSource(src); icp.setInputTarget(tgt); icp.align(unused, guess).  Points: float x,y,z at
 * byte offsets 0,4,8 of each stride; guess: optional row-major 4x4 (NULL = identity).  The caller
 * applies the acceptance test of PGO.cpp:385-387 (converged && fitness <= 0.3).  One launch: a persistent kernel that
 * occupies the whole device for the duration of the alignment (~0.5 ms).  Every kernel of this library that waits at a grid
 * barrier (this one and the cooperative VoxelGrid kernel behind rsx_voxelgrid_filter / rsx_loop_submap / rsx_loop_verify /
 * rsx_sc_add_keyframe) is ordered against the others ON THE DEVICE, across handles, streams and threads of one process
 * (csrc/rsx_persistent.h), and sizes its grid from the runtime's occupancy answer; two PROCESSES must not run such calls on
 * the same device at the same time (the barrier's 5 s watchdog turns that into RSX_ERR_HIP instead of a hang). */
int rsx_icp_align(rsx_icp *h, const void *src, size_t ns, size_t src_stride, const void *tgt, size_t nt, size_t tgt_stride,
                  const rsx_icp_params *params, const float *guess, rsx_icp_result *out);

/* ============================ keyframe clouds: loop verification and the map ==========================
 * What the pose-graph node does with the keyframe clouds it keeps (keyframeLaserClouds = the 0.4 m VoxelGrid output of
 * every keyframe, PGO.cpp:482-487), resident in HBM:
 *   rsx_loop_verify       = doICPVirtualRelative(loop, curr) (PGO.cpp:355-406): source = loopFindNearKeyframesCloud(curr, 0,
 *                           root = loop), target = loopFindNearKeyframesCloud(loop, 25, root = loop) -- keyframes
 *                           key - size .. key + size, EACH IN ITS OWN LOCAL FRAME, all moved by the one pose of the root
 *                           keyframe, concatenated, VoxelGrid 0.4 m (PGO.cpp:329-352) -- then ICP, the gate
 *                           `converged && fitness <= 0.3` (PGO.cpp:385), pcl::getTranslationAndEulerAngles and
 *                           poseFrom.between(poseTo) (PGO.cpp:400-407)
 *   rsx_kfstore_build_map = the cloud pubMap publishes (PGO.cpp:631-655): every SKIP_FRAMES-th keyframe through its own
 *                           pose, concatenated, VoxelGrid (host/pcd.h writes it to a .pcd file: the "resulting map save
 *                           function" of the reference's TODO list, README.md:139)
 * Poses are the reference's Pose6D: double x, y, z, roll, pitch, yaw (PGO.cpp:199-206).  PCL and GTSAM are not part of
 * the reference checkout; their pieces follow the published sources (oracle/loopverify_ref.c) -- parity unpinned; the
 * control flow is the reference's own.  Thread safety: one handle = one lock (the reference guards the same data with
 * mKF, PGO.cpp:339-341,486-495). */
typedef struct rsx_kfstore rsx_kfstore;

typedef struct {
  int32_t history_keyframe_search_num; /* 25: the target submap is loop - 25 .. loop + 25 (PGO.cpp:358) */
  float leaf;                          /* 0.4: downSizeFilterICP (PGO.cpp:687-689) */
  double fitness_threshold;            /* 0.3: loopFitnessScoreThreshold (PGO.cpp:384) */
  rsx_icp_params icp;                  /* PGO.cpp:374-378 */
} rsx_loop_verify_params;

typedef struct {
  int32_t accepted;    /* !(hasConverged() == false || getFitnessScore() > threshold)  (PGO.cpp:385) */
  int32_t converged, iterations, state; /* as rsx_icp_result */
  double fitness;
  float transform[16]; /* icp.getFinalTransformation(), row-major 4x4 */
  float x, y, z, roll, pitch, yaw; /* pcl::getTranslationAndEulerAngles of it (PGO.cpp:400-403) */
  double relative[16]; /* poseFrom.between(poseTo) with poseTo = identity (PGO.cpp:404-407), row-major 4x4: the loop factor */
  int64_t n_source, n_target; /* points of the two clouds after the VoxelGrid */
} rsx_loop_verify_result;

int rsx_kfstore_create(int device, rsx_kfstore **out);
int rsx_kfstore_destroy(rsx_kfstore *h);
/* keyframeLaserClouds.push_back(cloud) (PGO.cpp:487): n points stride_bytes apart, float x, y, z at byte offsets 0, 4, 8,
 * float intensity at intensity_offset (16 for pcl::PointXYZI; < 0: none, stored as 0).  The cloud is copied; *out_index =
 * its keyframe index.  _device: n packed float4 {x, y, z, intensity} already in this device's memory. */
int rsx_kfstore_add(rsx_kfstore *h, const void *pts, size_t n, size_t stride_bytes, int32_t intensity_offset, int32_t *out_index);
int rsx_kfstore_add_device(rsx_kfstore *h, const void *d_xyzi, size_t n, int32_t *out_index);
int rsx_kfstore_size(rsx_kfstore *h, int64_t *n_keyframes, int64_t *n_points);
/* keyframe `index` as packed float4; *out_count = its size (only the first max_out points are written) */
int rsx_kfstore_get(rsx_kfstore *h, int32_t index, float *out_xyzi, int64_t max_out, int64_t *out_count);
int rsx_loop_verify_default_params(rsx_loop_verify_params *p);
/* loopFindNearKeyframesCloud(out, key, submap_size, root) with root_pose6 = keyframePosesUpdated[root] (PGO.cpp:329-352) */
int rsx_loop_submap(rsx_kfstore *h, int32_t key, int32_t submap_size, const double *root_pose6, float leaf, float *out_xyzi,
                    int64_t max_out, int64_t *out_count);
/* doICPVirtualRelative(loop_idx, curr_idx) with root_pose6 = keyframePosesUpdated[loop_idx] (PGO.cpp:355-406);
 * params NULL = the reference's constants */
int rsx_loop_verify(rsx_kfstore *h, int32_t loop_idx, int32_t curr_idx, const double *root_pose6, const rsx_loop_verify_params *params,
                    rsx_loop_verify_result *out);
/* pubMap's cloud (PGO.cpp:631-655): keyframes 0, skip, 2 skip, ... < min(n_poses, stored), each through poses6[6 k .. 6 k + 5],
 * VoxelGrid `leaf`; *out_count = its size (only the first max_out points are written) */
int rsx_kfstore_build_map(rsx_kfstore *h, const double *poses6, int64_t n_poses, int32_t skip_frames, float leaf, float *out_xyzi,
                          int64_t max_out, int64_t *out_count);
/* CorAl alignment quality (above) of two stored keyframe clouds: A = keyframe idx_a, B = keyframe idx_b, each in its own frame and
 * read where the store keeps it (x and y of the packed float4); transform = the six doubles taking B into A's frame (NULL:
 * identity).  Synchronous, under the store's lock; both handles on one device; an index that is not stored gives
 * RSX_ERR_BAD_ARG; a keyframe above RSX_CORAL_MAX_POINTS points gives RSX_CORAL_STATUS_POINTS in *out_result */
int rsx_kfstore_alignment_quality(rsx_kfstore *kf, rsx_coral *h, int32_t idx_a, int32_t idx_b, const double *transform,
                                  const rsx_coral_params *params, rsx_coral_result *out_result);
/* downSizeFilterScancontext.filter + keyframeLaserClouds.push_back + scManager.makeAndSaveScancontextAndKeys in one call
 * (PGO.cpp:482-492): the downsampled cloud goes from the VoxelGrid into the keyframe store and the descriptor build
 * without leaving the GPU.  intensity_offset as above.  All three handles on the same device. */
int rsx_sc_add_keyframe(rsx_sc *h, rsx_voxelgrid *vg, rsx_kfstore *kf, const void *pts, size_t n, size_t stride_bytes,
                        int32_t intensity_offset, float leaf, int32_t *out_index);

#ifdef __cplusplus
}
#endif
#endif /* RSX_H */
