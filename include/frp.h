/* frp.h -- C ABI of the MI355X-native face-recognition hot path (libfrp.so).
 *
 * Drop-in boundary for the detect -> align -> embed -> match loop behind
 * backend/app/services/face_service.py of achiever04/face-recognition-platform.
 * The reference is pure Python and calls into un-vendored native packages; each
 * entry point below names the reference interface (file:line under /root/reference)
 * it replaces.  Plain C types only, no exceptions cross this boundary, every
 * function returns 0 on success or a negative frp_status; the message for the last
 * failure on a handle is available from frp_last_error().
 *
 * Ownership: the caller allocates and owns every in/out buffer (host pointers unless
 * the name says _device); the library owns what frp_create / frp_load_weights /
 * frp_gallery_* allocate and frees it in frp_destroy.
 * Threading: one handle = one HIP device + one private stream; calls on a handle are
 * serialised by an internal mutex (the reference fans out over a 4-thread pool,
 * backend/app/routes/camera.py:30,277-279 -- use one handle per GPU instead).
 * Gallery updates build a new device snapshot and swap it in, so a reader never sees
 * a half-updated matrix (the reference mutates state.ENCODINGS unlocked,
 * face_service.py:374,522).
 */
#ifndef FRP_H
#define FRP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FRP_EMB_DIM 512      /* embedding width (reference: 128-d dlib, face_service.py:179) */
#define FRP_CHIP 112         /* aligned face chip edge */
#define FRP_KPS 5            /* landmarks per face */
#define FRP_MAX_FACES_CAP 128
#define FRP_MAX_TOPK 64/* upper bound for max_faces per frame */

typedef enum frp_status {
    FRP_OK = 0,
    FRP_ERR_INVALID = -1,     /* bad argument / shape the kernels do not cover */
    FRP_ERR_HIP = -2,         /* a HIP runtime call failed (message has the hipError string) */
    FRP_ERR_NO_WEIGHTS = -3,  /* frp_load_weights has not succeeded on this handle */
    FRP_ERR_NO_GALLERY = -4,  /* match requested with an empty gallery */
    FRP_ERR_BLOB = -5,        /* malformed weight blob */
    FRP_ERR_OOM = -6
} frp_status;

typedef enum frp_dtype { FRP_F32 = 0, FRP_F16 = 1, FRP_F64 = 2 } frp_dtype;

/* process flags */
#define FRP_FLAG_FORCED_K 1u   /* take the top max_faces anchors by score: no threshold, no NMS
                                  (benchmark mode) */
#define FRP_FLAG_RGB 2u        /* input frames are RGB (face_recognition.load_image_file order,
                                  face_service.py:139) instead of BGR (cv2 capture order, camera.py:205) */
#define FRP_FLAG_NO_MATCH 4u   /* skip the gallery match (encode_face path, face_service.py:87-219) */
#define FRP_FLAG_WITHIN 8u     /* besides the top-1: per face the list of ALL gallery rows whose cosine is at or above the bound of
                                  frp_set_within, from the same gallery pass (frp_fetch_within; the caller's filter loop over every
                                  target, camera.py:246-256) */
#define FRP_FLAG_GROUPS 16u    /* the pass matches every face against the rows its FRAME's mask permits (frp_set_frame_groups) */
#define FRP_FLAG_TRACK 32u     /* face tracks: a detection that continues a track identified before gets the track's cached embedding
                                  and match, only the others are embedded (frp_track_config, frp_set_frame_streams) */
#define FRP_FLAG_JPEG_OPTIMIZE 64u   /* frp_encode_jpeg / frp_encode_jpeg_enhanced only: per-image optimal Huffman tables, the files
                                        of libjpeg's optimize_coding (Pillow's save(optimize=True)) */
#define FRP_GROUPS_ALL 0xFFFFFFFFu  /* member of every group: the mask of a row that arrived without one */

typedef struct frp_handle frp_handle;

typedef struct frp_config {
    int32_t struct_size;   /* sizeof(frp_config) */
    int32_t max_batch;     /* frames per call, default 32 */
    int32_t max_faces;     /* faces kept per frame, default 10 (camera.py:182,233-235) */
    int32_t max_h, max_w;  /* largest frame, default 1080 x 1920 */
    int32_t profile;       /* 1: time every stage with HIP events on the handle's stream */
    int32_t reserved[10];
} frp_config;

/* Per-stage GPU time (HIP events on the handle's stream, accumulated over calls since
 * the last frp_reset_counters; only filled when frp_config.profile = 1) and algorithmic work. */
typedef struct frp_counters {
    int32_t struct_size;
    int32_t calls;
    int64_t frames, faces;
    double ms_h2d, ms_preprocess, ms_det_conv, ms_decode, ms_align, ms_emb_conv, ms_l2norm, ms_match, ms_d2h;
    double ms_total;          /* first to last event of each call, summed */
    double det_conv_flops;    /* algorithmic 2*MAC of the detector conv launches (padding excluded) */
    double emb_conv_flops;    /* same for the embedder */
    int64_t det_conv_launches, emb_conv_launches;
    double match_bytes;       /* algorithmic gallery bytes streamed by the match kernel */
    int64_t match_launches;
    int64_t gallery_rows;
    double f8_conv_flops;     /* part of det/emb_conv_flops that ran on fp8 operands (BASELINE config 5) */
    int64_t f8_conv_launches;
    double reserved[6];
} frp_counters;

/* ---- lifecycle ------------------------------------------------------------------
 * replaces: module singleton construction `face_service = FaceService()`
 * (face_service.py:54-82,769) and the lazy model registry (state.py:135-259). */
int frp_create(int device, const frp_config* cfg, frp_handle** out);
void frp_destroy(frp_handle* h);
const char* frp_last_error(const frp_handle* h); /* valid until the next call on h */
const char* frp_version(void);

/* Weight blob (layout: include/frp_blob.h; produced by weights.pack_blob):
 * folded fp16 conv programs of the detector and the embedder.
 * replaces: insightface FaceAnalysis model-pack loading (deepfake_utils.py:39-51).
 * A failed load leaves the handle WITHOUT weights (FRP_ERR_NO_WEIGHTS on later compute calls), never with a
 * half-replaced program. */
int frp_load_weights(frp_handle* h, const void* blob, size_t bytes);

/* ---- gallery (watchlist embedding matrix) -----------------------------------------
 * replaces: state.ENCODINGS dict name -> list[float] (state.py:78) and its per-call
 * rebuild np.array([ENCODINGS[t] ...]) (face_service.py:409,461,558,595).
 * Rows are L2-normalised and stored as fp16 [N x 512] in HBM; names stay on the host. */
int frp_gallery_set(frp_handle* h, const void* emb, int64_t n, int32_t d, int32_t dtype);
/* rows already unit-norm fp16 in device memory of this handle's GPU (e.g. the output
 * of an RCCL all-gather); copied into a library-owned snapshot */
int frp_gallery_set_device(frp_handle* h, const void* dev_f16, int64_t n, int32_t d);
/* Zero-copy import of a matrix produced ON this GPU (the RCCL all-gather of the watch-list shards):
 * frp_gallery_reserve allocates a fresh, not yet visible snapshot of `capacity_rows` x 512 fp16 and returns its device
 * address; the caller (a collective, a kernel) fills rows [0, n) with UNIT fp16 rows and finishes its stream work;
 * frp_gallery_commit(n) makes it the gallery (n <= capacity; the old snapshot is released).  While a reservation is pending -
 * someone else (RCCL) may be writing into it - the other gallery updates (set, set_device, update_row, remove_row) FAIL with
 * FRP_ERR_INVALID and change nothing; frp_gallery_cancel discards the reservation (no-op without one); a second reserve
 * replaces the first. */
int frp_gallery_reserve(frp_handle* h, int64_t capacity_rows, void** dev_f16);
int frp_gallery_commit(frp_handle* h, int64_t n_rows);
int frp_gallery_cancel(frp_handle* h);
/* device address of the current snapshot (rows [0, frp_gallery_size)), valid until the next gallery update on this handle:
 * the source from which a second handle on the same GPU copies its own snapshot (frp_gallery_set_device) */
const void* frp_gallery_device_ptr(frp_handle* h);
int frp_gallery_update_row(frp_handle* h, int64_t row, const void* emb, int32_t d, int32_t dtype); /* row == size appends */
int frp_gallery_remove_row(frp_handle* h, int64_t row); /* last row moves into `row` (store/delete: face_service.py:374,522) */
int64_t frp_gallery_size(const frp_handle* h);
/* copy the normalised fp16 gallery back to the host (n_rows x 512 uint16) */
int frp_gallery_get(frp_handle* h, void* out_f16, int64_t first_row, int64_t n_rows);
/* Gallery groups: "who is looked for where" on ONE gallery (the reference's watchlist subset of the enrolled targets,
 * utils/db.py:493-510, alert_service.py; the mixed-camera batches of mixer.py / dist.py) instead of one gallery copy or one pass per
 * list, or a host filter behind an unrestricted match (wrong for top-1: the best row overall hides the best permitted one).
 * Every row carries a uint32 mask - bit g: member of group g - and every query one; row r is PERMITTED for query q iff
 * (row_groups[r] & q_groups[q]) != 0.  The grouped matches (frp_match_groups, frp_match_within_groups, a pass with FRP_FLAG_GROUPS)
 * are the ungrouped ones taken over the permitted rows only: same total order (cosine descending, row ascending), a NaN score never
 * selected, n_hits the true number of permitted rows at or above the bound, -1 / -2.0 for a query with nothing selectable (mask 0,
 * no permitted row, every score NaN) and for ranks past the number of permitted rows.  The cosine of a permitted row is the
 * frp_match_scores entry bit for bit; frp_match_scores and frp_gallery_distances ignore groups.
 * Rows that arrive without a mask have FRP_GROUPS_ALL: every row of frp_gallery_set / _set_device / _commit / _allgather (mask
 * changes are not replicated across ranks), a row appended by frp_gallery_update_row.  An overwrite keeps the row's mask and
 * frp_gallery_remove_row moves the last row's mask with the row.  Mask 0 is legal: the row is enrolled but matches nobody.
 * frp_gallery_set_groups / _get_groups: masks of rows [first_row, first_row + n_rows) within [0, frp_gallery_size);
 * FRP_ERR_INVALID for a null pointer or a range outside it, and - set_groups - while a reservation is pending. */
int frp_gallery_set_groups(frp_handle* h, const uint32_t* groups, int64_t first_row, int64_t n_rows);
int frp_gallery_get_groups(frp_handle* h, uint32_t* out, int64_t first_row, int64_t n_rows);

/* ---- exact rows for the REST-style compat path ---------------------------------------
 * replaces: the float64 arithmetic of face_recognition.face_distance on the rows AS ENROLLED
 * (np.linalg.norm(np.array([ENCODINGS[t] ...]) - q, axis=1): face_service.py:409-410,461-465,595-599, the 1-vs-1 calls of the
 * duplicate scan :357 and of cluster_faces :576).  The streaming loop matches on the unit fp16 rows (frp_match, the fused top-1 of
 * frp_process_*); compare_faces / find_k_nearest / batch_compare_faces / the duplicate scan report distances that must agree with
 * the reference's to 1e-6 - also for an exact copy (d = 0, where sqrt(2 - 2 cos) of fp16 rows reads 0.01-0.03), for d == tolerance,
 * for rows that are not unit vectors and for 128-d rows.
 * frp_gallery_exact(h, 1): from now on every row is ALSO kept as float64 [N x 512], exactly as handed to frp_gallery_set /
 * frp_gallery_update_row (dtype FRP_F64: bit for bit; FRP_F32 / FRP_F16: widened; not normalised; rows narrower than 512 are
 * zero-padded by the caller), 4 KB per row; rows that exist when it is switched on, and rows installed from device fp16 data
 * (frp_gallery_set_device, frp_gallery_commit), are the unit fp16 rows widened.  frp_gallery_exact(h, 0) frees the copy.
 * frp_gallery_distances: dist[m * n_cols + row] = ||row - q_m||_2 in float64 (differences, squares and sums in float64, one
 * correctly rounded sqrt; the summation order is fixed, so a result does not depend on N or M) for M queries of 512 doubles;
 * n_cols as in frp_match_scores.  frp_gallery_get_exact copies rows back (n_rows x 512 doubles). */
int frp_gallery_exact(frp_handle* h, int32_t on);
int frp_gallery_distances(frp_handle* h, const double* q, int32_t M, double* dist, int64_t n_cols);
int frp_gallery_get_exact(frp_handle* h, double* out, int64_t first_row, int64_t n_rows);

/* ---- gallery clustering ----------------------------------------------------------------
 * replaces: the greedy sweep of FaceService.cluster_faces (face_service.py:552-585) - in dict order the first unassigned name
 * becomes a seed and takes every unassigned name within the threshold - with the rows, the N x N scores and the labels all on the
 * device: one call, one int per name back.
 * The sweep runs in POSITIONS: order[p] is the gallery row of the p-th name (n distinct rows in [0, frp_gallery_size); after
 * frp_gallery_remove_row rows are no longer in enrolment order, so the permutation is an argument; n may be smaller than the
 * gallery: a subset is clustered among itself).  "Seed s takes p" is always evaluated with s as the QUERY and p's row as the
 * column - the fp16 scores are not symmetric, a query is normalised and rounded again - on the very numbers the stand-alone calls
 * return:   default              cos >= min_cos  in float32, cos = the frp_match_scores entry of s's unit fp16 row (widened,
 *                                normalised and rounded as frp_match_scores does with a query) against row order[p], bit for bit
 *           FRP_CLUSTER_EXACT    dist <= max_dist in float64, dist = the frp_gallery_distances entry of s's float64 row
 * The bound that is not in use is ignored; a NaN score never passes and a NaN bound passes nothing.  A seed always takes itself,
 * whatever its own score is: a zero or NaN row is a cluster of one.
 * seed_pos[p] = the position of the seed that took p (== p for a seed); *n_clusters = the number of seeds.  Seeds arise in ascending
 * position, so cluster k is the k-th seed and its members, in ascending position behind the seed, are the reference's list.
 * tile: candidate seeds scored per gallery pass, 1..FRP_CLUSTER_MAX_TILE (0: the largest); the result does not depend on it.
 * Waits for the stream; changes no gallery state, no result of the last pass and no track.  The fp16 route's passes count in
 * match_launches / match_bytes.  FRP_ERR_NO_GALLERY for an empty gallery; FRP_ERR_INVALID - nothing launched, nothing written - for
 * a null pointer, n <= 0 or beyond the gallery size, a row out of range or listed twice, a tile out of range, an unknown flag and
 * FRP_CLUSTER_EXACT without exact rows. */
#define FRP_CLUSTER_EXACT 1u   /* sweep the float64 rows (frp_gallery_exact must be on): member iff dist <= max_dist */
#define FRP_CLUSTER_MAX_TILE 64
int frp_gallery_cluster(frp_handle* h, const int32_t* order, int64_t n, float min_cos, double max_dist,
                        int32_t tile /* 1..64, 0: 64 */, uint32_t flags, int32_t* seed_pos /* [n] */, int32_t* n_clusters);

/* ---- the hot path -----------------------------------------------------------------
 * replaces, per frame: cv2.cvtColor(BGR2RGB) (camera.py:225), face_recognition.face_locations
 * (camera.py:232, face_service.py:156), the max_faces cap (camera.py:233-235),
 * face_recognition.face_encodings (camera.py:237, face_service.py:179), and per face
 * FaceService.compare_faces + the caller's filter loop reduced to top-1
 * (face_service.py:395-443, camera.py:243-259).
 *
 * bgr: B frames of H x W x 3 u8, row_stride bytes between rows, frames contiguous
 * (frame b starts at bgr + b*H*row_stride).  Outputs (any may be NULL):
 *   boxes  [B*K*4]  x1,y1,x2,y2 in frame pixels     kps [B*K*10]  5 x (x,y)
 *   scores [B*K]    sigmoid of the anchor logit      counts [B]   faces kept (<= K = max_faces)
 *   emb    [B*K*512] unit embeddings                 match_idx [B*K] gallery row of the best
 *   match_cos [B*K] its cosine (distance = sqrt(max(0, 2-2cos)))      cosine, -1 if no gallery
 * Slots k >= counts[b] are zero-filled (match_idx -1). */
int frp_process_frames(frp_handle* h, const uint8_t* bgr, int32_t B, int32_t H, int32_t W, int64_t row_stride,
                       int32_t max_faces, float det_thresh, float nms_iou, uint32_t flags,
                       float* boxes, float* kps, float* scores, int32_t* counts,
                       float* emb, int32_t* match_idx, float* match_cos);

/* Same pipeline split for callers that keep frames resident in HBM (the benchmark's timed
 * region starts with inputs already on the device): upload once, process many, fetch. */
int frp_upload_frames(frp_handle* h, const uint8_t* bgr, int32_t B, int32_t H, int32_t W, int64_t row_stride);
int frp_process_resident(frp_handle* h, int32_t max_faces, float det_thresh, float nms_iou, uint32_t flags);
/* B, max_faces: the shape the caller's buffers were sized for; FRP_ERR_INVALID when the handle's last results have
 * another shape (a concurrent caller replaced them) -- nothing is written then */
int frp_fetch_results(frp_handle* h, int32_t B, int32_t max_faces, float* boxes, float* kps, float* scores, int32_t* counts,
                      float* emb, int32_t* match_idx, float* match_cos);
int frp_synchronize(frp_handle* h);
/* Radius match of the streaming passes (FRP_FLAG_WITHIN of frp_process_frames / frp_process_resident / frp_finish_faces): which
 * enrolled rows lie within tolerance of a face, not only which one is nearest
 * -> the filter `d <= tolerance` over all targets (camera.py:246-256; d <= tol <=> cos >= 1 - tol^2 / 2 on unit rows).
 * frp_set_within stores the bound (min_cos >= -2, not NaN) and the list size (1 <= cap <= FRP_MAX_TOPK) for the flagged passes
 * that follow; a flagged pass without it fails with FRP_ERR_INVALID.  The pass launches the same match kernel it would have
 * launched, with an epilogue that lists (row, cosine) of every score >= min_cos; top-1, embeddings and everything else are
 * unchanged, and without the flag nothing is.
 * frp_fetch_within (B, max_faces checked as in frp_fetch_results, cap against the pass): per face slot n_hits [B*K] = the TRUE
 * number of rows at or above the bound - it may exceed cap - and idx / cos [B*K x cap] = the first min(n_hits, cap) of them by
 * (cosine descending, row ascending), -1 / -2.0 beyond; slots k >= counts[b], and every slot of a pass that did not match (no
 * gallery, FRP_FLAG_NO_MATCH), give n_hits 0.  A cosine equals the frp_match_scores entry of that embedding's fp16 query bit for
 * bit.  The list of a face with n_hits > cap is rebuilt here, from the embeddings the pass left on the device (one score row per
 * such face + the top-k selection); FRP_ERR_INVALID if a later match / embed call on the handle has replaced them. */
int frp_set_within(frp_handle* h, float min_cos, int32_t cap);
/* Grouped passes (FRP_FLAG_GROUPS of frp_process_frames / frp_process_resident / frp_finish_faces / frp_process_pyramid): masks [B],
 * one per FRAME, for the flagged passes that follow - every face of frame b is matched against the rows masks[b] permits (frame mask
 * 0: its faces match nothing, -1).  The pass launches the GROUPS form of the match kernel it would have launched, once; detections,
 * embeddings and everything else are unchanged, and without the flag nothing is.  With FRP_FLAG_WITHIN the lists of frp_fetch_within
 * are the grouped ones, a rebuilt list included.  A flagged pass fails with FRP_ERR_INVALID, nothing launched and the last pass's
 * results still fetchable, without a preceding frp_set_frame_groups, with a B other than the pass's, or together with
 * FRP_FLAG_NO_MATCH.  frp_counters.match_bytes of a grouped launch counts N * (1024 + 4). */
int frp_set_frame_groups(frp_handle* h, const uint32_t* masks, int32_t B);
int frp_fetch_within(frp_handle* h, int32_t B, int32_t max_faces, int32_t cap, int32_t* idx, float* cos, int32_t* n_hits);

/* Face tracks (FRP_FLAG_TRACK of frp_process_frames / frp_process_resident / frp_finish_faces): the workload is video, a stream's
 * consecutive frames show the same faces in almost the same place, and the embedder is the dominant cost of a step - so a flagged
 * pass decides ON THE DEVICE which detections continue a face identified before, embeds only the others (the embed list and its
 * count stay in device memory, as in every threshold pass) and gives the rest the bits their track cached.
 * State per stream: next_id and an ordered list of at most FRP_TRACK_SLOTS = 128 entries {box, id, age (frames of the stream since the
 * embedding the entry carries was computed), missed, match_idx, match_cos, emb[512]}.  One frame of stream s (a stream's frames are
 * taken in batch order), detections j = 0 .. n-1 in detector order, n = clamp(counts[b], 0, max_faces):
 *   1. j ascending, over the entries no earlier j claimed: IoU as the NMS kernels compute it (+1-pixel areas, fp32, one rounding
 *      per operation, inter / ((a + b) - inter)); candidates have iou >= iou_min (a NaN fails); the largest IoU wins, a tie goes to
 *      the lowest entry.  Matched: the detection inherits the id, a = age + 1; a < refresh and the pass not stale: REUSED - it carries
 *      the entry's emb / match_idx / match_cos, age = a; otherwise embedded, age 0.  Unmatched: id = next_id++, embedded, age 0.
 *   2. the new list: the n detections in order (missed 0), then the unclaimed entries in their old order with missed + 1 and
 *      age + 1 while missed <= max_missed, cut at 128.
 * A frame of stream -1 embeds every detection, reports track_id -1 and touches no state; streams absent from a batch keep theirs.
 * The source of a reused slot is an entry of the state before the pass or a face embedded EARLIER IN THE SAME BATCH (frame 2 of a
 * stream reusing what frame 1 computes), resolved behind the matcher.  frp_fetch_results then gives every live slot its emb / idx /
 * cos: embedded slots their own, reused slots the bits of their source.
 * `stale`: set by frp_track_config, by every gallery mutation (set, set_device, commit, update_row, remove_row, allgather,
 * set_groups) and by frp_gallery_exact; the next flagged pass then embeds every face (ids continue) and clears it - a cached
 * match_idx never outlives a row move.
 * Passes without the flag are unchanged whether or not tracking is configured, and leave the track state alone.
 * frp_counters.faces and the embedder's FLOP count keep meaning EMBEDDED faces; frp_track_stats has both totals.
 * Refused with FRP_ERR_INVALID before anything is launched, overwritten or advanced: the flag without frp_track_config, without
 * frp_set_frame_streams for the pass's B, together with FRP_FLAG_WITHIN or FRP_FLAG_GROUPS, passed to frp_process_pyramid, or to
 * frp_finish_faces without boxes.  Grouped / within passes and the pyramid pass under tracking are follow-ups.
 *
 * frp_track_config: iou_min in (0, 1], refresh >= 1, max_missed >= 0, max_streams 1..64: allocates the tables, clears every track,
 * sets stale.  max_streams = 0 releases everything and turns tracking off.  (Callers' usual values 0.3 / 8 / 2 are ordinary
 * defaults, not measured optima.) */
#define FRP_TRACK_MAX_STREAMS 64
int frp_track_config(frp_handle* h, int32_t max_streams, float iou_min, int32_t refresh, int32_t max_missed);
/* the stream of every frame, entries in [-1, max_streams), for the flagged passes that follow (life cycle of frp_set_frame_groups) */
int frp_set_frame_streams(frp_handle* h, const int32_t* stream_of_frame, int32_t B);
/* forget the tracks of one stream (a camera reconnect), -1: of all; ids start at 0 again */
int frp_track_reset(frp_handle* h, int32_t stream);
/* [B x max_faces] of the last flagged pass: track id (-1: untracked frame or no face), 1 where the result was reused, age; the
   shape check of frp_fetch_results */
int frp_fetch_tracks(frp_handle* h, int32_t B, int32_t max_faces, int32_t* track_id, int32_t* reused, int32_t* age);
/* faces embedded / reused by flagged passes since the last frp_track_config (device totals: waits for the stream) */
int frp_track_stats(frp_handle* h, int64_t* embedded, int64_t* reused);
/* the real associate / compact / resolve / store launches on host detections (parity tests; needs no weights, advances the handle's
   track state, honours and clears stale): streams [B], boxes [B][K][4], counts [B]; emb_in [B][K][512], idx_in, cos_in [B][K] stand in
   for what the embedder and matcher would produce for the slots that turn out embedded (compacted here in face_slot order).
   Out: track_id, reused, age [B][K]; face_slot [B x K] (-1 behind n_embed); emb [B][K][512], idx, cos [B][K]; slots beyond the
   counts are zero / -1 */
int frp_debug_track_step(frp_handle* h, const int32_t* streams, const float* boxes, const int32_t* counts, int32_t B, int32_t K,
                         const float* emb_in, const int32_t* idx_in, const float* cos_in, int32_t* track_id, int32_t* reused,
                         int32_t* age, int32_t* face_slot, int32_t* n_embed, float* emb, int32_t* idx, float* cos);

/* Overlapped ingest for streaming callers (the camera loop keeps producing frames while the previous
 * batch is on the GPU, camera.py:277-305): the NEXT batch is copied host -> device on a private copy
 * stream into a staging buffer while the resident batch is being processed; frp_swap_frames makes the
 * staged batch the resident one (stream-ordered, no host wait).  The copy only overlaps when `bgr` is
 * page-locked: frp_host_alloc hands out such memory (freed by frp_host_free or with the handle).
 *     upload_async(t+1); process_resident(t); fetch_results(t); swap_frames(); ...                  */
void* frp_host_alloc(frp_handle* h, size_t bytes);
void frp_host_free(frp_handle* h, void* p);
int frp_upload_frames_async(frp_handle* h, const uint8_t* bgr, int32_t B, int32_t H, int32_t W, int64_t row_stride);
int frp_swap_frames(frp_handle* h);

/* ---- encoded stills ------------------------------------------------------
 * replaces: the image decode behind the upload routes - face_recognition.load_image_file (PIL) at
 * backend/app/services/face_service.py:139 and backend/app/routes/face.py:177-185,216,404,976.  Baseline JPEG (8-bit, Huffman,
 * one interleaved scan; grayscale, 4:4:4, 4:2:2, 4:2:0): the bit stream - the one serial part - is decoded on host threads
 * into quantised DCT coefficients in page-locked memory; dequantisation, the inverse DCT (the integer "slow" algorithm of
 * libjpeg, bit for bit), the triangle-filter chroma upsampling and YCbCr -> BGR run on the GPU, on the handle's copy stream,
 * and write the staging frame buffer of frp_upload_frames_async.  Progressive / arithmetic-coded / 12-bit files are refused. */
typedef struct frp_jpeg_info {
    int32_t width, height, components;      /* 1 (grayscale) or 3 (YCbCr) */
    int32_t h_samp[3], v_samp[3];           /* sampling factors per component (chroma always 1 x 1) */
    int32_t mcus_x, mcus_y;                 /* MCU grid (MCU = 8 h_samp[0] x 8 v_samp[0] pixels) */
    int32_t restart_interval, progressive;
} frp_jpeg_info;
/* header only; needs no handle.  FRP_ERR_INVALID for what the decoder does not cover. */
int frp_jpeg_info_get(const uint8_t* data, size_t size, frp_jpeg_info* info);
/* host entropy decode alone (parity tests, no handle): coef = per component [blocks_y][blocks_x][64] int16 in natural order,
 * quantised, components back to back (blocks_x = mcus_x * h_samp[c], blocks_y = mcus_y * v_samp[c]); qtab [3][64] */
int frp_jpeg_coefficients(const uint8_t* data, size_t size, int16_t* coef, size_t coef_elems, uint16_t* qtab, frp_jpeg_info* info);
/* B stills of identical geometry -> the staging frame buffer [B, height, width, 3] u8 BGR (grayscale: replicated), as
 * frp_upload_frames_async does for raw frames: follow with frp_swap_frames.  Returns when the coefficients are staged; the
 * device half runs asynchronously on the copy stream. */
int frp_upload_jpeg_async(frp_handle* h, const uint8_t* const* jpegs, const size_t* sizes, int32_t B);
/* network passes replayed from a captured hipGraph so far (round 5: a detector / embedder pass asked for a second time with the same shapes,
 * buffers and switches is captured and from then on replayed by one call; FRP_NO_GRAPH turns that off) - tests and diagnosis */
int64_t frp_debug_graph_replays(frp_handle* h);
/* diagnostic: batches of this handle whose ENTROPY decode ran on the device too (every frame carries restart intervals of at most 32
 * MCUs - one thread per interval; longer intervals: the host decoder, unless FRP_JPEG_DEVICE_HUFFMAN=1; =0: always the host) */
int64_t frp_debug_jpeg_device_batches(frp_handle* h);
/* Entropy decode on the device for frames WITHOUT restart markers (what PIL, cv2 and most Motion-JPEG cameras write): the
 * self-synchronising decoder.  The scan is cut into subsequences, every one is decoded speculatively by a thread of its own, and entry
 * states are handed from subsequence to subsequence until nothing changes - the fix-point is the serial decode, bit for bit; damaged
 * streams are refused by the call as on the host path.  Opt-in per handle: on != 0 makes frp_upload_jpeg_async take it for every batch
 * whose frames all have restart_interval == 0 (mixed batches and restart-interval batches route as before); default 0, or 1 for handles
 * created while FRP_JPEG_SELFSYNC is set (to something not starting with '0'; read once per process).  on > 1 (measurements): on, with
 * subsequences of `on` bytes - a multiple of 16 in 16 .. 1024 - instead of the product's size; anything else is FRP_ERR_INVALID. */
int frp_set_jpeg_selfsync(frp_handle* h, int32_t on);
/* diagnostic: batches of this handle decoded by it (frp_debug_jpeg_device_batches counts restart-interval batches only) */
int64_t frp_debug_jpeg_selfsync_batches(frp_handle* h);
/* parity: the same decode alone, B stills of identical geometry without restart markers -> coef = the quantised coefficients of every image
 * in the layout of frp_jpeg_coefficients, one image after the other (coef_elems >= B times one image's).  subseq_bytes: the subsequence
 * size, a multiple of 16 in 16 .. 1024, or 0 for the one frp_upload_jpeg_async uses.  stats (may be NULL): [B][4] = subsequences,
 * synchronisation rounds (<= subsequences), blocks counted (at most the image's total), error flag - filled also when the call refuses the
 * batch for a corrupt image (FRP_ERR_INVALID, "JPEG i: ...").  Needs no weights; a staged batch stays staged. */
int frp_jpeg_selfsync_coefficients(frp_handle* h, const uint8_t* const* jpegs, const size_t* sizes, int32_t B, int32_t subseq_bytes, int16_t* coef,
                                   int64_t coef_elems, int32_t* stats);

/* ---- decoded video surfaces ----------------------------------------------
 * replaces: the frames cv2.VideoCapture hands out for "device ID, RTSP URL, or HTTP stream" sources (routes/camera.py:52), for callers
 * that bring their own decoder.  The library ships no codec; every decoder (a hardware video block, VA-API, ffmpeg in software) emits
 * 8-bit YUV 4:2:0 surfaces with row pitches, and these calls take them - from host memory at 1.5 bytes per pixel over PCIe instead of
 * the 3 of BGR, or where they already lie in device memory - and convert them on the GPU into the BGR frames the pipeline keeps
 * resident.
 * A frame is a Y plane [height][width] plus chroma at half resolution in both directions; width and height must be even.  Chroma is
 * REPLICATED: pixel (x, y) uses the sample at (x >> 1, y >> 1), no siting filter.  Exact integer arithmetic; with u = U - 128,
 * v = V - 128, >> an arithmetic shift and clamp to 0 .. 255:
 *   FRP_YUV_BT601 / FRP_YUV_BT709 (limited "video" range):   y = max(0, Y - 16) * CY
 *       R = clamp((y + CVR * v + 2^19) >> 20)   G = clamp((y - CVG * v - CUG * u + 2^19) >> 20)   B = clamp((y + CUB * u + 2^19) >> 20)
 *       the constants are round(c * 2^20) of the usual three-decimal coefficients -
 *       601: CY 1220542 (1.164), CVR 1673527 (1.596), CVG 852492 (0.813), CUG 409993 (0.391), CUB 2116026 (2.018)
 *       709: CY 1220542,         CVR 1880097 (1.793), CVG 558891 (0.533), CUG 223347 (0.213), CUB 2214593 (2.112)
 *   FRP_YUV_JFIF (full range, libjpeg's rule - what the JPEG ingest applies):
 *       R = clamp(Y + ((91881 * v + 32768) >> 16))   G = clamp(Y + ((-22554 * u - 46802 * v + 32768) >> 16))
 *       B = clamp(Y + ((116130 * u + 32768) >> 16))
 * These formulas are the contract.  The 601 constants are believed to be OpenCV's (COLOR_YUV2BGR_NV12); parity with cv2 is neither
 * claimed nor tested. */
#define FRP_YUV_NV12 0       /* Y plane, then one plane of interleaved U,V */
#define FRP_YUV_NV21 1       /* Y plane, then one plane of interleaved V,U */
#define FRP_YUV_I420 2       /* Y, U, V planes */
#define FRP_YUV_YV12 3       /* Y, V, U planes */
#define FRP_YUV_BT601 0
#define FRP_YUV_BT709 1
#define FRP_YUV_JFIF 2
#define FRP_YUV_DEVICE 1     /* frp_yuv_desc.flags: the plane pointers are device memory of the handle's GPU */
typedef struct frp_yuv_desc {
    int32_t struct_size, layout, matrix, flags;   /* sizeof(frp_yuv_desc), FRP_YUV_NV12 ..., FRP_YUV_BT601 ..., 0 or FRP_YUV_DEVICE */
    int32_t width, height;                         /* even, width * height <= 2^30 */
    int64_t y_pitch, c_pitch;                      /* bytes per row of the Y plane / of each chroma plane (NV12 / NV21: of the UV plane) */
} frp_yuv_desc;
/* planes: [B][3] pointers per frame, the planes in the order the layout names them - Y, U, V for FRP_YUV_I420; Y, V, U for
 * FRP_YUV_YV12; Y, the interleaved plane, NULL for NV12 / NV21.  Frames may lie anywhere: there is no frame stride.  1 <= B <= 1024.
 * A bad argument is FRP_ERR_INVALID with a message that names the field; nothing is queued then and a staged batch stays staged.
 * Host sources (pageable or page-locked; only page-locked memory overlaps with compute) are copied plane by plane into a packed device
 * buffer; device sources are read in place through their pitches.
 * LIFETIME of the surfaces, host and device alike: complete before the call.  The blocking call has read them when it returns.  The
 * staged call only QUEUES its copies and its kernel on the copy stream and returns at once: the surfaces must stay untouched - not
 * refilled by the decoder, not freed - until frp_swap_frames has been called AND a call that waits for the compute stream
 * (frp_fetch_results, frp_synchronize) has returned - the pipeline's own order.
 * frp_upload_yuv: blocking, on the compute stream, the batch is resident on return (as frp_upload_frames).  frp_upload_yuv_async: staged
 * on the copy stream (as frp_upload_frames_async): follow with frp_swap_frames. */
int frp_upload_yuv(frp_handle* h, const frp_yuv_desc* desc, const uint8_t* const* planes, int32_t B);
int frp_upload_yuv_async(frp_handle* h, const frp_yuv_desc* desc, const uint8_t* const* planes, int32_t B);
/* the resident BGR frames as they lie, frames [first, first + n) of the batch -> out (n * H * W * 3 bytes; parity tests, snapshots).
 * Waits for the compute stream; needs no weights.  FRP_ERR_INVALID when nothing is resident, when the range is empty or outside the
 * batch, or when out_bytes is too small. */
int frp_get_frames(frp_handle* h, uint8_t* out, int64_t out_bytes, int32_t first, int32_t n);

/* ---- multi-GPU: one process per GPU, ONE collective ----------------------------------------------------
 * Frames are sharded one stream per GPU and never exchanged.  The watch list is: every rank builds (decrypts) rows
 * [rank * ceil(N / R), ...) and the unit fp16 matrix is all-gathered over RCCL / xGMI straight into a reserved snapshot of
 * every rank's handle, then committed - replaces the single in-process dict of the reference (backend/app/state.py:78,
 * rebuilt per call at face_service.py:409).  The library owns the collective (librccl opened at first use); the launcher
 * only carries the 128-byte unique id from rank 0 to the other ranks (any control channel: a file, MPI, torch.distributed
 * object broadcast - frp_amd/dist.py). */
#define FRP_DIST_ID_BYTES 128
/* rank 0: a fresh communicator id */
int frp_dist_unique_id(void* id128);
/* collective over `world` ranks (each on its own GPU): creates this handle's communicator */
int frp_dist_init(frp_handle* h, const void* id128, int32_t rank, int32_t world);
int frp_dist_destroy(frp_handle* h);
/* collective: `shard` = this rank's rows [shard_rows, 512] in HOST memory (dtype FRP_F32 / FRP_F16 / FRP_F64 as
 * frp_gallery_set; normalised on upload), shard_rows = min(block, n_total - rank * block) with block = ceil(n_total / world).
 * On return every rank's gallery is the full [n_total, 512] matrix, rows in rank order. */
int frp_gallery_allgather(frp_handle* h, const void* shard, int64_t shard_rows, int32_t dtype, int64_t n_total);

/* ---- stage entry points (REST paths and parity tests) ------------------------------- */
/* detection only -> face_recognition.face_locations (camera.py:232) */
int frp_detect(frp_handle* h, const uint8_t* bgr, int32_t B, int32_t H, int32_t W, int64_t row_stride,
               int32_t max_faces, float det_thresh, float nms_iou, uint32_t flags,
               float* boxes, float* kps, float* scores, int32_t* counts, int32_t* anchor_idx);
/* Multi-scale pyramid building blocks (BASELINE config 4: "RetinaFace multi-scale pyramid"):
 * detect on the RESIDENT frames bilinearly resized to det_h x det_w (== frame size: no resize); boxes and
 * landmarks come back in the coordinates of the resized image.  The caller merges the scales
 * (pyramid.merge_scales) and hands the merged landmarks to frp_finish_faces, which aligns from the
 * full-resolution resident frames, embeds and matches.  counts[b] <= max_faces faces per frame. */
int frp_detect_resident(frp_handle* h, int32_t B, int32_t det_h, int32_t det_w, int32_t max_faces, float det_thresh, float nms_iou,
                        uint32_t flags, float* boxes, float* kps, float* scores, int32_t* counts, int32_t* anchor_idx);
/* the u8 frames the detector last read (the resident frames or their resize), [B, hs, ws, 3] (parity tests) */
int frp_get_det_source(frp_handle* h, uint8_t* out, int64_t out_bytes, int32_t* hs, int32_t* ws);
/* B: the resident batch the face list and the output buffers were sized for (checked under the handle mutex) */
int frp_finish_faces(frp_handle* h, int32_t B, const float* boxes, const float* kps, const float* scores, const int32_t* counts,
                     int32_t max_faces, uint32_t flags, float* emb, int32_t* match_idx, float* match_cos);
/* the whole pass on the resident frames: per scale resize + detector + decode/NMS (threshold mode, per_scale slots),
   cross-scale merge + NMS on the device, then align / embed / match from the FULL-RESOLUTION frames with the face count
   left in device memory.  Asynchronous like frp_process_resident; results through frp_fetch_results(B, max_faces)
   (boxes / kps / scores / counts in frame pixels), hit lists through frp_fetch_within.
   The merge equals pyramid.merge_scales bit for bit: coordinates times (float)W / (float)det_w resp. (float)H / (float)det_h in one
   fp32 multiply, no clipping; scale order, then detector order, score descending, ties to the earlier; the +1-pixel-area greedy NMS.
   FRP_ERR_INVALID: no weights, no resident frames, n_scales outside 1..4, per_scale or max_faces outside 1..128,
   n_scales * per_scale > 512, a size outside 1..16384, FRP_FLAG_FORCED_K (a forced top-K per scale has no meaning under a merge),
   FRP_FLAG_WITHIN without frp_set_within; nothing of the last pass is overwritten then.  FRP_FLAG_RGB, FRP_FLAG_NO_MATCH and
   FRP_FLAG_WITHIN mean what they mean to frp_process_resident; the embedder's kernel family follows B * max_faces, as for every
   process call.
   The call leaves the detector source at the LAST scale: frp_get_det_source and frp_get_head_map report that scale, and the next
   frp_process_frames / frp_process_resident switches back to full size by itself.
   Stage timers: the stages still add up to ms_total.  ms_det_conv and ms_decode hold the last scale's detector and its decode + the
   merge; everything the earlier scales ran (resize, detector, decode) is counted, with the last scale's resize, in ms_preprocess. */
int frp_process_pyramid(frp_handle* h, int32_t n_scales, const int32_t* det_hw /* [n_scales][2]: h, w */, int32_t per_scale,
                        int32_t max_faces, float det_thresh, float nms_iou, uint32_t flags);
/* the merge launch alone on caller-supplied detections (host arrays, scale-major [n_scales][B][per_scale]...): needs neither
   weights nor resident frames.  counts[s][b] must lie in [0, per_scale] and the scores of live rows must be finite and >= 0
   (FRP_ERR_INVALID otherwise); the last pass's results stay as they are (parity tests) */
int frp_debug_pyramid_merge(frp_handle* h, int32_t n_scales, const int32_t* det_hw, int32_t B, int32_t per_scale,
                            int32_t frame_h, int32_t frame_w, const float* boxes, const float* kps, const float* scores,
                            const int32_t* counts, int32_t max_faces, float nms_iou,
                            float* out_boxes, float* out_kps, float* out_scores, int32_t* out_counts);

/* the embedder's tail alone on host operands (parity tests): the FC as the pipeline launches it - a 1x1 conv with fp32 output, split
 * over K where the pass's own choice splits it - and the l2norm kernel behind it; needs neither weights nor resident frames.
 * x [cap, K] fp16, w [D, K] fp16, bias [D] fp32 (K and D multiples of 8, D <= 1024; a split needs K % 64 == 0), n <= cap rows exist.
 * mode FRP_FC_HOST_COUNT: launched for n rows with the factor of n chosen on the host, as a forced-K process call does;
 *      FRP_FC_DEVICE_COUNT: launched for the capacity with n in device memory, both kernels choose the factor there (threshold mode);
 *      1: no split - the conv's fp32 epilogue adds the bias, the plain l2norm; s >= 2: the factor s (FRP_ERR_INVALID where the conv
 *      launch refuses it: s must divide K / 64).
 * flags: bits 17 / 18 of frp_conv2d_nhwc (the tile class; an fp32-output launch takes the 256-pixel tiles whatever they say).
 * emb [cap, D] fp32 and emb_f16 [cap, D]: the slab workspace and both outputs are filled with 0xFF bytes on the device before the
 * launches, so a slab read without having been written shows as NaN and the rows at or beyond n come back as 0xFF.  n == 0 with a
 * host count launches nothing.  *n_cu: the handle's compute units; *host_factor: the factor the host's rule gives n rows (1: none).
 * FRP_ERR_INVALID - nothing launched - for n > cap, D > 1024 and anything else out of range. */
#define FRP_FC_HOST_COUNT 0
#define FRP_FC_DEVICE_COUNT (-1)
int frp_debug_fc_l2norm(frp_handle* h, const void* x_f16, const void* w_f16, const float* bias, int32_t cap, int32_t n, int32_t K,
                        int32_t D, int32_t mode, int32_t flags, float* emb, void* emb_f16, int32_t* n_cu, int32_t* host_factor);

/* raw detector head maps of the last detect/process call, per stride level 0..2:
 * [B, H/stride, W/stride, 32] fp16 (parity tests) */
int frp_get_head_map(frp_handle* h, int32_t level, void* out_f16, int64_t out_bytes, int32_t* hl, int32_t* wl);
/* diagnostic: runs the detector program on the resident frames up to and including op n_ops - 1 and returns that op's
 * output [B, th, tw, tc] fp16 (out_f16 NULL: dimensions only, the prefix still runs).  Buffers are shared between tensors,
 * so an inner tensor is only readable from a prefix run (tools/det_bisect.py: per-layer determinism / parity bisection).
 * While the two stems run as one kernel (the default) op 0's map never reaches memory: n_ops == 1 fails with
 * FRP_ERR_INVALID unless FRP_NO_FUSED_STEM12 is set; n_ops == 2 is then the output of that one kernel */
int frp_debug_det_prefix(frp_handle* h, int32_t n_ops, void* out_f16, int64_t out_bytes, int32_t* th, int32_t* tw, int32_t* tc);
/* diagnostic: enable != 0 - every later detector pass hashes each op's output right behind the op (one 64-bit slot per op,
 * 64 slots); out64 != NULL receives the hashes of the last pass (tools/det_hash_bisect.py: which op of a FULL pass differed) */
int frp_debug_det_hashes(frp_handle* h, int32_t enable, uint64_t* out64);
/* decode + NMS on caller-supplied head maps [B,H_l,W_l,32] fp16 (parity tests) */
int frp_decode_heads(frp_handle* h, const void* head8, const void* head16, const void* head32,
                     int32_t B, int32_t canvas_h, int32_t canvas_w, int32_t max_faces, float det_thresh, float nms_iou,
                     uint32_t flags, float* boxes, float* kps, float* scores, int32_t* counts, int32_t* anchor_idx);
/* 5-landmark similarity warp -> normalised chips [M,112,112,8] fp16 (channels R,G,B,0..)
 * -> insightface norm_crop behind face_encodings (camera.py:237) */
int frp_align(frp_handle* h, const uint8_t* bgr, int32_t H, int32_t W, int64_t row_stride,
              const float* kps, int32_t M, uint32_t flags, void* chips_f16);
/* diagnostic: the pipeline's own align launch (compacted face list, frame of each slot, frame stride) on the RESIDENT frames [B,H,W,3]
 * for caller-supplied landmarks kps [B, max_faces, 10] and counts [B]; no weights needed.  device_count == 0: launched for
 * sum(counts) faces; != 0: launched for the capacity B * max_faces with the count read from device memory, as the threshold-mode
 * pipeline does.  chips_f16 receives all B * max_faces chips [112,112,8] fp16 (out_bytes >= that): the first sum(counts), frame-major,
 * are the aligned faces, every chip behind them holds the fill 0xFFFF (parity tests) */
int frp_debug_align_resident(frp_handle* h, const float* kps, const int32_t* counts, int32_t max_faces, uint32_t flags,
                             int32_t device_count, void* chips_f16, int64_t out_bytes);
/* diagnostic: the matcher on M queries handed over as fp16 bits [M x 512] - copied as they are, NOT normalised - against the gallery.
 * n_device < 0: the count M is a launch argument; with `scores` (M x n_cols floats, n_cols as in frp_match_scores) the per-tile kernel
 * and its score matrix, without it the kernel frp_match(topk = 1) would take (FRP_MATCH_V1 is honoured).  n_device >= 0: launched for
 * the capacity M with the count n_device <= M read from device memory, as the threshold-mode pipeline does; FRP_ERR_INVALID where
 * that form does not exist (with `scores`, more than 512 queries after rounding up to 32, FRP_MATCH_V1 set).  idx / cos [M]: the
 * device buffers are filled with 0xFF bytes before the launch, so an entry the kernels did not write reads -1 / 0xFFFFFFFF (parity tests) */
int frp_debug_match_f16(frp_handle* h, const void* q_f16, int32_t M, int32_t n_device, int32_t* idx, float* cos, float* scores,
                        int64_t n_cols);
/* aligned u8 BGR chips [M,112,112,3] -> unit embeddings [M,512] */
int frp_embed_aligned(frp_handle* h, const uint8_t* chips, int32_t M, float* emb);
/* landmarks on one frame -> unit embeddings [M,512] (face_encodings with known faces) */
int frp_embed_faces(frp_handle* h, const uint8_t* bgr, int32_t H, int32_t W, int64_t row_stride,
                    const float* kps, int32_t M, uint32_t flags, float* emb);
/* cosine top-k (1 <= topk <= FRP_MAX_TOPK) of M queries vs the gallery, ordered by (cosine descending, row
 * ascending): idx / cos are [M x topk]; entries beyond the gallery size are -1 / -2.0.  A NaN score is never selected: a query
 * with a NaN or an infinite component (its normalised row holds a NaN) gets -1 / -2.0 in every entry, for topk == 1 as well
 * (the same "nothing here" as frp_match_within's list tails), and a gallery row that holds a NaN is never returned
 * -> face_recognition.face_distance + argmin / argpartition (face_service.py:410,599-603) */
int frp_match(frp_handle* h, const float* q, int32_t M, int32_t topk, int32_t* idx, float* cos);
/* all cosines [M x N] (the N-dict compat path of compare_faces, face_service.py:409-432) */
/* n_cols: the gallery size cos_all was sized for; FRP_ERR_INVALID (nothing written) when the gallery has another size
 * by the time the call holds the handle -- re-read frp_gallery_size and retry */
int frp_match_scores(frp_handle* h, const float* q, int32_t M, float* cos_all, int64_t n_cols);
/* radius match: every gallery row whose cosine with a query is >= min_cos (min_cos >= -2, not NaN; -2 lists every row), M host
 * queries normalised on upload as in frp_match, 1 <= cap <= FRP_MAX_TOPK.  n_hits [M] = the true number of such rows (may exceed
 * cap); idx / cos [M x cap] = the first min(n_hits, cap) of them by (cosine descending, row ascending) - what frp_match(topk = cap)
 * lists, cut at the bound - and -1 / -2.0 beyond; cosines bit-identical to frp_match_scores.  One gallery pass with the hit lists
 * written by the match kernel's epilogue (M <= 512: the persistent kernel; above: the per-tile kernel, in chunks of 65536
 * queries): no M x N matrix exists unless a query has more than cap hits - its list, and only its, is rebuilt from its score row.
 * -> compare_faces' `d <= tolerance` over all targets, batch_compare_faces (face_service.py:409-432,448-481) */
int frp_match_within(frp_handle* h, const float* q, int32_t M, float min_cos, int32_t cap, int32_t* idx, float* cos, int32_t* n_hits);
/* frp_match / frp_match_within over the rows each query's mask permits (q_groups [M]; semantics: frp_gallery_set_groups above).  The
 * same kernels in their GROUPS form: an accumulator element whose row is not permitted is set to the value rows past the gallery's
 * end get, ahead of the selection; topk > 1 and a list with n_hits > cap select from score rows that hold a NaN where a row is
 * not permitted.  Arguments are checked as in the ungrouped calls (null pointers, topk, cap, min_cos) before anything is launched. */
int frp_match_groups(frp_handle* h, const float* q, int32_t M, const uint32_t* q_groups, int32_t topk, int32_t* idx, float* cos);
int frp_match_within_groups(frp_handle* h, const float* q, int32_t M, const uint32_t* q_groups, float min_cos, int32_t cap,
                            int32_t* idx, float* cos, int32_t* n_hits);

/* Face quality: the blur and lighting sums of rectangles of the RESIDENT frames (those of the last frp_upload_frames / frp_swap_frames /
 * frp_process_frames), as uploaded.
 * replaces the pixel half of FaceService.assess_face_quality (face_service.py:276-297): the grey conversion, cv2.Laplacian and the
 * mean / variance passes over the crop.  rects [n*5] = frame, top, right, bottom, left (the css order of face_locations); per
 * rectangle sums [n*4] = S1, S2, L1, L2 = sum g, sum g^2, sum lap, sum lap^2 over the crop's pixels, with
 * g = (R*4899 + G*9617 + B*1868 + 8192) >> 14 (R and B by FRP_FLAG_RGB, the only flag allowed) and lap = up + down + left + right -
 * 4*centre on g, BORDER_REFLECT_101 at the edges of the crop.  Exact integers: var(g) = (N*S2 - S1^2) / N^2 for the N pixels of the
 * crop, the Laplacian's variance alike.  Queued on the handle's stream behind a pending pass; waits; the handle's last results stay
 * fetchable (frp_fetch_results, frp_fetch_within).  n == 0: FRP_OK, nothing launched.  FRP_ERR_INVALID - nothing launched, nothing
 * written, the message names the rectangle - without resident frames, for n < 0, another flag, or a rectangle outside
 * 0 <= frame < B, 0 <= top < bottom <= H, 0 <= left < right <= W. */
int frp_face_quality(frp_handle* h, const int32_t* rects, int32_t n, uint32_t flags, int64_t* sums);

/* JPEG encoder: rectangles of the RESIDENT frames (as for frp_face_quality) -> baseline JPEG files, one per rectangle, with libjpeg's
 * integer arithmetic at its defaults (jccolor / jcsample / jfdctint / jcdctmgr, Annex K tables scaled by `quality`, one interleaved
 * Huffman scan): byte for byte the scan PIL / cv2.imencode writes for the same pixels.
 * replaces: cv2.imencode('.jpg', frame) of the multipart /feed (routes/camera.py:73-87) and of /snapshot (camera.py:148-149) - and
 * the 6.2 MB per 1080p frame that had to cross PCIe before a host encoder could run.
 * subsampling: FRP_JPEG_420 (what cv2 and PIL write by default) or FRP_JPEG_444.  restart_mcus = r > 0: DRI = r MCUs, RSTm markers. */
#define FRP_JPEG_420 420
#define FRP_JPEG_444 444
/* The segments in front of the scan, in PIL's order: SOI, APP0 (JFIF 1.01), DQT 0, DQT 1, SOF0, DHT DC0 AC0 DC1 AC1, DRI (r > 0 only), SOS.
 * Needs no handle.  Returns the byte count (<= 1024), or FRP_ERR_INVALID - nothing written - when cap is too small or an argument is
 * out of range (width / height 1..65535, quality 1..100, restart_mcus 0..65535). */
int64_t frp_jpeg_encode_headers(int32_t width, int32_t height, int32_t quality, int32_t subsampling, int32_t restart_mcus, uint8_t* out, int64_t cap);
/* libjpeg's jpeg_gen_optimal_table (T.81 K.2 with libjpeg's conventions): the symbol counts freq [256] -> BITS bits [16] (codes of
 * length 1..16) and HUFFVAL vals [256] (the symbols by code length, then by value; the first `return value` entries are set) of the
 * length-limited Huffman code a DHT segment carries.  A pseudo-symbol of count 1 keeps every real symbol off the all-ones code; the
 * two least frequent entries merge, ties going to the larger symbol; lengths beyond 16 are shortened as in Figure K.3.  Needs no
 * handle.  Returns the number of symbols with a non-zero count, or FRP_ERR_INVALID - nothing written - for a null argument, counts
 * that are all zero, or a code deeper than 32 bits before limiting (where libjpeg gives up too). */
int frp_jpeg_optimal_table(const uint32_t freq[256], uint8_t bits[16], uint8_t vals[256]);
/* rects [n*5] = frame, top, right, bottom, left, validated as in frp_face_quality (the message names the rectangle); pixels are BGR,
 * RGB with FRP_FLAG_RGB.  out: the n complete files back to back; offsets [n+1]: offsets[i] = where file i
 * starts, offsets[n] = the total.  When the total exceeds out_cap: FRP_ERR_INVALID, offsets filled, out untouched - call again with
 * room for offsets[n].  n == 0: FRP_OK, nothing launched.  Any argument out of range: FRP_ERR_INVALID, nothing launched, nothing
 * written.  Queued on the handle's stream behind a pending pass; waits; the handle's last results stay fetchable.
 * FRP_FLAG_JPEG_OPTIMIZE (the only other flag allowed): every file gets Huffman tables of its own, made from the counts of its own
 * symbols (a histogram kernel, frp_jpeg_optimal_table on the host, per-image tables in the entropy stage and in the four DHT
 * segments) - byte for byte Pillow's save(quality=q, optimize=True), one more wait inside the call, everything else as without the
 * flag.  Pillow cannot write every such file: with optimize its output buffer is max(65536, w*h) bytes (2*w*h at quality >= 95) and
 * libjpeg cannot suspend ("Suspension not allowed here", e.g. 160 x 160 noise at quality 100, 4:4:4); this encoder has no such limit. */
int frp_encode_jpeg(frp_handle* h, const int32_t* rects, int32_t n, int32_t quality, int32_t subsampling, int32_t restart_mcus, uint32_t flags,
                    uint8_t* out, int64_t out_cap, int64_t* offsets);
/* parity: the symbol counts FRP_FLAG_JPEG_OPTIMIZE builds its tables from - per image FRP_JPEG_HIST_ELEMS counts: dc [2][16] by
 * magnitude category (table 0: Y, table 1: Cb and Cr together), then ac [2][256] by run / size symbol (0x00 = EOB, 0xF0 = ZRL);
 * hist_elems must be n * FRP_JPEG_HIST_ELEMS.  flags: FRP_FLAG_RGB; FRP_FLAG_JPEG_OPTIMIZE is accepted and changes nothing.  With
 * frp_jpeg_optimal_table a failing file can be traced to the kernel or to the table generator. */
#define FRP_JPEG_HIST_ELEMS 544
int frp_encode_jpeg_histograms(frp_handle* h, const int32_t* rects, int32_t n, int32_t quality, int32_t subsampling, int32_t restart_mcus,
                               uint32_t flags, uint32_t* hist, int64_t hist_elems);
/* parity: the quantised coefficients of the same rectangles before entropy coding - int16, natural order, per image the layout of
 * frp_jpeg_coefficients (per component [blocks_y][blocks_x][64] over the MCU-padded grid, components back to back), one image after
 * the other; coef_elems must be their exact number */
int frp_encode_jpeg_coefficients(frp_handle* h, const int32_t* rects, int32_t n, int32_t quality, int32_t subsampling, uint32_t flags,
                                 int16_t* coef, int64_t coef_elems);

/* Snapshot enhancer: rectangles of the RESIDENT frames, each upscaled to its own output size with Pillow's Image.resize(BICUBIC) and
 * sharpened with ImageFilter.UnsharpMask(radius, percent, threshold) - Pillow's integer arithmetic on 8-bit pixels, byte for byte.
 * replaces: the enhance=true branch of /snapshot (routes/snapshot.py:54-117 -> services/enhancer.py:64-92): resize x2 capped at
 * ENHANCER_MAX_PIXELS, UnsharpMask(1, 120, 3), JPEG at quality 85 - and the trip of the frame to a host thread in front of it.
 * rects [n*5] as for the JPEG encoder; sizes [n*2] = out_w, out_h per rectangle.  An axis with out == in is not resampled (as in
 * Pillow); with sharpen == 0 the mask is skipped.  The blur clamps at the edge of the enhanced crop, never at the frame's: a crop's
 * neighbours in the frame do not reach the result.
 * Refused with FRP_ERR_INVALID before anything is launched, nothing written, the message names the rectangle: a rectangle the JPEG
 * encoder refuses; out_w < w or out_h < h (no downscaling); out_w or out_h above 65535; out_w * out_h above
 * FRP_ENHANCE_MAX_PIXELS; radius < 0, NaN or above FRP_ENHANCE_MAX_RADIUS; percent < 0; threshold < 0; a flag other than
 * FRP_FLAG_RGB; no resident frames; n < 0.  n == 0: FRP_OK, nothing launched.  Queued on the handle's stream behind a pending
 * pass; waits; the handle's last results stay fetchable. */
typedef struct frp_enhance_params {
    float radius;          /* UnsharpMask radius, 0..FRP_ENHANCE_MAX_RADIUS */
    int32_t percent;       /* >= 0 */
    int32_t threshold;     /* >= 0: differences up to it are left alone */
    int32_t sharpen;       /* 0: resample only */
} frp_enhance_params;
#define FRP_ENHANCE_MAX_RADIUS 2.0f
#define FRP_ENHANCE_MAX_PIXELS 16777216   /* per output image */
/* out: the n images back to back, each [out_h][out_w][3] tightly packed in the frames' channel order (FRP_FLAG_RGB changes nothing
 * here); offsets [n+1]: byte offsets, offsets[n] = the total.  When the total exceeds out_cap: FRP_ERR_INVALID, offsets filled, out
 * untouched. */
int frp_enhance_pixels(frp_handle* h, const int32_t* rects, const int32_t* sizes, int32_t n, const frp_enhance_params* params, uint32_t flags,
                       uint8_t* out, int64_t out_cap, int64_t* offsets);
/* the same images as baseline JPEG files - quality, subsampling, restart_mcus, flags, out, out_cap and offsets as in the JPEG encoder,
 * whose checks apply too: byte for byte Pillow's save(quality=q) of the enhanced image, with FRP_FLAG_JPEG_OPTIMIZE Pillow's
 * save(quality=q, optimize=True), which is the file the reference writes (services/enhancer.py:88).  The two differ in the DHT
 * segments and the scan's codes; every quantised coefficient agrees.  The encoder reads the enhanced pixels where the enhancer left
 * them: no pixel crosses PCIe between the two. */
int frp_encode_jpeg_enhanced(frp_handle* h, const int32_t* rects, const int32_t* sizes, int32_t n, const frp_enhance_params* params, int32_t quality,
                             int32_t subsampling, int32_t restart_mcus, uint32_t flags, uint8_t* out, int64_t out_cap, int64_t* offsets);

/* one convolution through the MFMA kernel on host tensors (kernel parity tests):
 * x [N,H,W,Cin] fp16, w [Cout][k][k][Cin] fp16, bias fp32 [Cout] or [9][Cout], out fp16 or fp32
 * flags (0: what the engine would launch for this shape, as set by the environment switches of INTEGRATION.md):
 *   bit 0      bias [9][Cout], one row per border class of the output pixel
 *   bit 1      fp32 output
 *   bit 2      res [N,res_h,res_w,Cout] at half resolution, upsampled x2 on the fly
 *   bit 8      the generic kernel, also where a specialised one covers the shape
 *   bit 9      lab build: the first-generation row-patch kernel's pre-prefetch k-step
 *   bits 9-12  lab build: the number of a timing ablation of the Winograd kernel
 *   bits 10-13 lab build: the number of a timing ablation of the first-generation row-patch kernel (wrong results)
 *   bit 13     lab build: the Winograd kernel with one wave per SIMD
 *   bit 14     head outputs (Cout <= 32) on all 64 rows of the tile; lab build: the first-generation row-patch / Winograd kernels
 *   bit 15     64-cout layers in 256-pixel tiles; lab build: the Winograd kernel's first-generation k-loop
 *   bit 16     through the Winograd kernel (an error where it does not cover the shape), never in quarter tiles
 *   bit 17/18  quarter tiles (128 pixels x 64 couts) always / never; default: by the tile count
 *   bit 19     lab build: the Winograd kernel's 2-D tiles whatever the shape
 *   bit 20     not the 64 -> 64 register-resident kernel
 *   bit 21     the opt-in stride-2 row-patch kernel
 *   bit 22     the 64 -> 64 kernel with all waves in the same order (A/B of its ping-pong schedule)
 * (bits 8-15 and 19-22: csrc/frp_internal.h, CONV_DBG_*) */
int frp_conv2d_nhwc(frp_handle* h, const void* x, int32_t N, int32_t H, int32_t W, int32_t Cin,
                    const void* w, int32_t Cout, int32_t ksize, int32_t stride,
                    const float* bias, const float* slope, const void* res, int32_t res_h, int32_t res_w,
                    int32_t act, int32_t flags, void* out);

/* one residual block of two 3x3 stride-1 64 -> 64 convolutions through the fused block kernel (csrc/conv3x3_block64.hip; kernel parity
 * tests): out = act2(conv2(act1(conv1(x))) + x) on host tensors, x and out [N,H,W,64] fp16, w1 / w2 [64][3][3][64] fp16, bias1 [64] fp32
 * ([9][64] with FRP_FLAG_BORDER_BIAS = 1 in flags1), bias2 [64], slopes [64] or NULL.  The two epilogue combinations of the networks:
 * (act1, flags1, act2) = (ReLU, 0, ReLU) and (PReLU, border bias, none); anything else, or a shape beyond signed 32-bit byte offsets, is
 * FRP_ERR_INVALID.  On the device x and out lie between guard regions filled with fp16 NaNs: a read outside x poisons the result, a
 * write outside out is reported as FRP_ERR_HIP. */
int frp_conv_block64(frp_handle* h, const void* x, int32_t N, int32_t H, int32_t W, const void* w1, const float* bias1,
                     const float* slope1, int32_t act1, int32_t flags1, const void* w2, const float* bias2, const float* slope2,
                     int32_t act2, void* out);

/* one 3x3 stride-1 convolution on fp8 operands through the block-scaled fp8 MFMA kernel (BASELINE config 5; kernel parity
 * tests): x8 [N,H,W,Cin] and w8 [Cout][3][3][Cin] are OCP E4M3 bytes (Cin a multiple of 128), value = code * scale with
 * one scale per output channel (wscale) and one for the input tensor (in_scale); res16 fp16 or NULL; `out` fp16, or E4M3
 * bytes (value / out_scale) with FRP_FLAG_OUT_FP8 = 64 in `flags`; out2_f8: optional E4M3 copy of an fp16 output */
int frp_conv2d_f8(frp_handle* h, const void* x8, int32_t N, int32_t H, int32_t W, int32_t Cin, const void* w8, int32_t Cout,
                  const float* wscale, const float* bias, const float* slope, const void* res16, int32_t act, int32_t flags,
                  float in_scale, float out_scale, void* out, void* out2_f8);

/* ---- observability ---------------------------------------------------------------
 * replaces: FaceService._metrics / get_performance_metrics (face_service.py:69-77,636-656) */
int frp_get_counters(frp_handle* h, frp_counters* out);
int frp_reset_counters(frp_handle* h);
/* switch the per-stage HIP-event timing (frp_config.profile) on or off.  frp_process_resident leaves its events unread; they
 * are read by the next call that waits for the stream anyway (frp_fetch_results, frp_synchronize) or, with a wait of its own,
 * by the first other call that would re-record them.  frp_upload_frames_async / frp_swap_frames never wait for them. */
int frp_set_profile(frp_handle* h, int32_t on);

#ifdef __cplusplus
}
#endif
#endif /* FRP_H */
