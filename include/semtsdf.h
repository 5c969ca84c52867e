/*
 * semtsdf.h — C ABI of the MI355X-native semantic TSDF engine (libsemtsdf.so).
 *
 * This is the drop-in boundary for the fusion hot path of qq456cvb/SLAM-MaskRCNN:
 *   - the C++ class `TSDF` of src/SfM_CUDA (tsdf.cuh:7-67, tsdf.cu:137-540) and the
 *     `Viewer` raycast (viewer.cu:17-179), and
 *   - the pybind11 extension `tsdf_cuda.tsdf_update` of src/TSDF_Python
 *     (tsdf.cpp:11-33, module tsdf.cpp:35-37).
 * Every entry point is `extern "C"`, takes plain pointers and sizes, and returns an
 * `int` status (SEMTSDF_OK == 0).  On failure `semtsdf_last_error()` returns a
 * thread-local message.  Host pointers are borrowed for the duration of the call; the
 * library owns all device memory it allocates.  `stream` arguments are `hipStream_t`
 * passed as `void*` (NULL = the handle's own stream).
 *
 * Volume layout at this boundary (TSDF_Python tsdf.py:48-52, SfM tsdf.cu:55): flat
 *   x-major, z fastest, idx = x*Dy*Dz + y*Dz + z.  sdf f32, weight i32, colour u8x3 (SfM)
 *   or i32x3 (TSDF_Python), histogram 32 x u32 per voxel.  The device storage is private:
 *   1x8x32 tiles of 256 voxels, histogram bin-major;
 *   semtsdf_download()/semtsdf_upload() convert to and from the reference layouts.
 */
#ifndef SEMTSDF_H
#define SEMTSDF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SEMTSDF_ABI_VERSION 12
#define SEMTSDF_MAX_OBJECTS 32 /* tsdf.cuh:4 */

/* ---- status codes ------------------------------------------------------------ */
#define SEMTSDF_OK 0
#define SEMTSDF_ERR_INVALID (-1)     /* bad argument, shape or parameter */
#define SEMTSDF_ERR_HIP (-2)         /* a HIP runtime call failed (message has the HIP error) */
#define SEMTSDF_ERR_OOM (-3)         /* device allocation failed */
#define SEMTSDF_ERR_LABEL (-4)       /* a mask label >= SEMTSDF_MAX_OBJECTS (tsdf.cu:61 UB in the reference) */
#define SEMTSDF_ERR_STATE (-5)       /* call out of order (e.g. raycast on a sharded handle) */
#define SEMTSDF_ERR_COMM (-6)        /* collective failure */
#define SEMTSDF_ERR_UNSUPPORTED (-7) /* feature not available for this handle/mode */
#define SEMTSDF_NEED_PIXELS 1        /* semtsdf_shard_assoc_apply: the decision needs the per-pixel
                                        data of every shard (semtsdf_shard_assoc_pixels) */

/* ---- volume flags -------------------------------------------------------------- */
#define SEMTSDF_F_SEMANTIC 0x1u   /* 32-bin per-voxel instance histogram (SfM tsdf.cu:61) */
#define SEMTSDF_F_GATE_COLOR 0x2u /* colour+histogram only when f < gate (SfM tsdf.cu:57) */
#define SEMTSDF_F_COLOR_I32 0x4u  /* colour int32x3 (TSDF_Python tsdf.py:50) instead of u8x3 */
#define SEMTSDF_F_VOTE 0x8u       /* label vote tsdf_cls/tsdf_cls_cnt (TSDF_Python/tsdf.cu:48-57) */
#define SEMTSDF_F_NO_CULL 0x10u   /* disable brick frustum/depth culling (debug; same results) */
/* Instance ids past the histogram (a deviation, opt-in).  The reference hands every unmatched
 * label the id num_objs++ (tsdf.cu:379-383) without a bound, and its integrate then counts an
 * id >= 32 in the bins of the next voxel (tsdf.cu:61, out of bounds).  By default the engine
 * keeps the reference's ids (the u8 mask holds them modulo 256, as mask_ptr[i] = num_objs does),
 * drops the histogram votes of ids >= 32 (counted in semtsdf_state::label_votes_dropped) and
 * reports SEMTSDF_ERR_LABEL from the synchronous calls of the frame that minted one; the handle
 * stays usable.  With SEMTSDF_F_ID_SATURATE an unmatched label that would get an id >= 32 is
 * relabelled 0 (background) instead, num_objs stops at 32 and no error is reported. */
#define SEMTSDF_F_ID_SATURATE 0x20u

/* ---- placement modes (a1) ---------------------------------------------- */
#define SEMTSDF_PLACE_SFM 0    /* SfM tsdf.cu:173-199: f32, depth->u8 saturates, mean in metres */
#define SEMTSDF_PLACE_PYTHON 1 /* TSDF_Python tsdf.py:32-47: f64, depth->u8 wraps mod 256 */

/* ---- raycast render modes (a8) ------------------------------------------------------ */
#define SEMTSDF_RENDER_LABEL 0 /* argmax instance -> palette BGR (viewer.cu:71-79) */
#define SEMTSDF_RENDER_COLOR 1 /* trilinear colour at the hit (tsdf_render.frag:125-131) */

typedef struct semtsdf_params {
    int32_t dim[3];          /* global volume dims (Dx, Dy, Dz); reference: 256^3 (tsdf.cuh:52) */
    float vol_start[3];      /* world position of voxel (0,0,0) (tsdf.cu:195) */
    float vol_end[3];        /* world position of voxel (D-1) (tsdf.cu:196) */
    float voxel[3];          /* (vol_end - vol_start)/(D-1) (tsdf.cu:197) */
    float mu;                /* truncation, 5*voxel.x (tsdf.cu:199) */
    float K[16];             /* row-major 4x4 intrinsic (tsdf.cu:143-146) */
    float Kinv[16];          /* its inverse (tsdf.cu:147) */
    int32_t width, height;   /* frame size (640x480) */
    float depth_scale;       /* raw depth units per metre: 5000 (tsdf.cu:49) */
    float gate;              /* colour/histogram gate on f: 0.99 (tsdf.cu:57) */
    float box_thresh;        /* association box-mask threshold: 0.3 (tsdf.cu:128) */
    float prior_mrcnn_err_rate; /* Configuration::prior_mrcnn_err_rate = 0.05 (configuration.h:8);
                                   must lie in [2^-10, 1) */
    float duplicate_thresh;  /* Configuration::duplicate_thresh = 0.5 (configuration.h:9; unused upstream) */
    uint32_t flags;          /* SEMTSDF_F_* */
    /* Z-slab sharding.  The global z axis is cut into chunks of z_chunk
     * planes, dealt round by round in boustrophedon order: with n = z_nshards, chunk c of
     * round r = c / n, position k = c % n, is owned by shard k (r even) or n - 1 - k (r odd).
     * z_nshards == 1 -> whole volume
     * (z_chunk is then ignored).  Sharded handles store one extra halo plane per chunk. */
    int32_t z_shard, z_nshards, z_chunk;
} semtsdf_params;

typedef struct semtsdf_vol semtsdf_vol; /* opaque volume handle */

typedef struct semtsdf_state {
    uint32_t n_obs;          /* integrated frames used by association (tsdf.cuh:46) */
    int32_t num_objs;        /* next global instance id (tsdf.cuh:61) */
    int32_t local_dim[3];    /* stored dims on this device (z includes halo planes) */
    uint64_t local_voxels;   /* local_dim product */
    uint64_t device_bytes;   /* bytes of device memory owned by the handle */
    uint64_t label_votes_dropped; /* histogram votes of ids >= 32 dropped by the integrate since the
                                     last reset: the id policy without SEMTSDF_F_ID_SATURATE (with
                                     the flag no such id is minted and this stays 0) */
} semtsdf_state;

/* Per-frame association result (filter_overlaps tsdf.cu:304-416). */
typedef struct semtsdf_assoc_stats {
    int32_t max_obj_now;                /* max(mask)+1 of the incoming mask */
    int32_t num_objs;                   /* after relabel */
    int32_t assigned_prev[SEMTSDF_MAX_OBJECTS]; /* current label i -> previous id, or -1 */
    float assigned_prob[SEMTSDF_MAX_OBJECTS];   /* exp(A/C) of the accepted match */
    uint8_t lut[256];                   /* old label -> new label applied to the mask */
    uint32_t exact_rows;                /* bit i: current label i was decided from its exact f32
                                           pixel-order sums (the rows the fixed-point certificate
                                           could not decide) */
    uint32_t reject_rows;               /* bit i: the certificate proved every candidate of label i
                                           at or below 3 * prior for every f32 rounding of its sums:
                                           rejected (a new id) without the exact path */
} semtsdf_assoc_stats;

/* Accumulated kernel timings (HIP events on the launch stream). */
typedef struct semtsdf_timing {
    double integrate_ms;  /* sum over integrate kernel launches */
    double assoc_ms;      /* sum over association (march+accumulate+decide+relabel) */
    double render_ms;     /* sum over raycast render launches */
    uint64_t n_integrate, n_assoc, n_render;
    uint64_t touched;     /* voxels updated (count mode only) */
    uint64_t gated;       /* voxels whose colour/histogram were updated (count mode only) */
    uint64_t bricks;      /* integrate units that survived the frustum/depth cull (count mode only) */
    double prep_ms;       /* sum over the per-frame depth-pyramid + brick-cull passes */
    uint64_t n_prep;
    uint64_t free_units;  /* of those, units whose touched voxels all have f == 1 (count mode only) */
    uint64_t full_units;  /* of those, free units whose every voxel is touched (no projection; count mode only) */
    uint64_t lazy_voxels; /* always 0: counted the lazy-weight experiment's voxels (removed);
                             the field stays for the ABI */
    uint64_t assoc_exact_frames; /* association decisions that took the exact f32 path (always counted) */
    uint64_t assoc_exact_rows;   /* rows decided on it, summed over those decisions */
    uint64_t touched_lines;      /* 128-B lines of the sdf array (8 y x 4 z voxels of a tile) holding a
                                    touched voxel: the line-granular floor of the state traffic (count mode only) */
    double assoc_pos_max;        /* largest positive association term log(p / n_obs) any decision saw
                                    (p > n_obs; 0: none); from log 32 on every row takes the exact path */
} semtsdf_timing;

/* ---- library ------------------------------------------------------------------------ */
const char* semtsdf_last_error(void);
int semtsdf_abi_version(void);
/* SHA-256 (hex) of the sources, hipcc flags and compiler version the library was built from
 * (__graft_entry__.build_key): the key PMC traffic records are stamped with. */
const char* semtsdf_build_key(void);
int semtsdf_device_count(int* out);
int semtsdf_set_device(int device);
int semtsdf_stream_create(void** out_stream);
int semtsdf_stream_destroy(void* stream);
int semtsdf_stream_sync(void* stream);
int semtsdf_dev_malloc(void** out, size_t bytes);
int semtsdf_dev_free(void* ptr);
/* kind: 1 = host->device, 2 = device->host, 3 = device->device (async on stream);
 * 4 = a copy kernel on stream reading a device-accessible source (pinned host memory),
 *     16-B aligned pointers and size: does not block the calling thread */
int semtsdf_memcpy(void* dst, const void* src, size_t bytes, int kind, void* stream);

/* ---- parameters / placement (a1) --------------------------------------------------- */
/* Fill defaults: K from (fx, fy, cx, cy) as tsdf.cu:137-147, constants of §a10, cubic dim. */
int semtsdf_params_default(semtsdf_params* p, int dim, const float intrinsics[4], int width, int height);
/* Place the volume from the first frame's depth (tsdf.cu:173-199 / tsdf.py:32-47).
 * mean_depth is in metres for SEMTSDF_PLACE_SFM and in raw depth units for
 * SEMTSDF_PLACE_PYTHON (tsdf.py:38-40). Writes vol_start, vol_end, voxel, mu. */
int semtsdf_place_from_frame(semtsdf_params* p, const uint16_t* depth, double mean_depth, int mode);

/* ---- volume lifecycle ------------------------------------------------------------- */
int semtsdf_create(const semtsdf_params* p, int device, semtsdf_vol** out);
int semtsdf_destroy(semtsdf_vol* v);
int semtsdf_get_params(const semtsdf_vol* v, semtsdf_params* out);
int semtsdf_get_state(const semtsdf_vol* v, semtsdf_state* out);
int semtsdf_set_state(semtsdf_vol* v, uint32_t n_obs, int32_t num_objs);
void* semtsdf_get_stream(const semtsdf_vol* v);
/* sdf := mu (metres, tsdf.cu:243-244), weight/colour/histogram := 0, n_obs = num_objs = 0. */
int semtsdf_reset(semtsdf_vol* v, void* stream);
/* Move the volume by whole 8^3 bricks so that it follows the camera (no reference counterpart).
 * shift = (sx, sy, sz) in voxels, each a multiple of 8 with |s| < 2^20.  Afterwards the voxel at
 * index i holds what the voxel at i + s held -- sdf, weight, colour, all 32 histogram bins, the
 * label vote -- in the storage form it had; a voxel whose source i + s lies outside [0, dim) on any
 * axis holds what semtsdf_reset leaves (sdf = mu, everything else 0).  The placement moves with it,
 * rounded once from double: vol_start[a] = (float)((double)vol_start[a] + (double)s[a] *
 * (double)voxel[a]), vol_end likewise; semtsdf_get_params returns it and every later call uses it.
 * Poses are relative to frame 0 (E = W2C_k * W2C_0^-1), not to vol_start, so they stay valid.
 * voxel, mu, dim, n_obs, num_objs, the weight bound, the storage forms and the dropped-vote counter
 * do not change.  The empty-space maps are rebuilt by the next march and the steady flags cleared,
 * as after semtsdf_upload.  |s[a]| >= dim[a] is legal: the whole volume becomes the reset state and
 * the counters keep their values.  (0, 0, 0) does nothing and returns SEMTSDF_OK.
 * The call orders itself after the work queued on the handle (as semtsdf_reset and semtsdf_upload
 * do), runs on `stream` and synchronises before it returns.  It holds at most 16 bytes per stored
 * voxel of extra device memory while it runs (counted in device_bytes, released before return).
 * Errors, decided before any device work: a NULL argument, a component that is not a multiple of
 * 8 or with |s| >= 2^20, a new placement that is not finite: SEMTSDF_ERR_INVALID; a Z-sharded
 * handle: SEMTSDF_ERR_STATE.  SEMTSDF_ERR_OOM from the first allocation leaves the volume as it
 * was; a failure later in the call leaves voxel contents that only semtsdf_reset or a full
 * semtsdf_upload make defined again. */
int semtsdf_shift(semtsdf_vol* v, const int32_t shift[3], void* stream);

/* ---- integrate (a4) ------------------------------------------------------------------
 * One frame into the volume: E = extrinsic * init_extrinsic_inv (row-major 4x4 f32,
 * tsdf.cu:217).  depth u16 [H*W], rgb u8 [H*W*3], mask u8 [H*W] (may be NULL unless
 * SEMANTIC).  In a SEMANTIC volume every integrated frame is an observation, as every
 * integrated frame of the reference advances n_obs_ (tsdf.cu:218-220): the first one (n_obs ==
 * 0) sets num_objs = max(mask) + 1 (tsdf.cu:463-468), and each one advances n_obs by 1, so
 * semtsdf_associate + semtsdf_integrate leave the state semtsdf_parse_frame leaves (ABI 12; up
 * to ABI 11 only parse_frame advanced n_obs).  Mask labels >= 32: without
 * SEMTSDF_F_ID_SATURATE their histogram votes are dropped and counted and the host-pointer
 * call reports SEMTSDF_ERR_LABEL after applying the frame in full; with it they are refused
 * (SEMTSDF_ERR_LABEL, nothing applied). */
int semtsdf_integrate(semtsdf_vol* v, const uint16_t* depth, const uint8_t* rgb,
                      const uint8_t* mask, const float E[16], void* stream);
/* Same with device pointers (inputs already resident in HBM). */
int semtsdf_integrate_dev(semtsdf_vol* v, const uint16_t* depth_d, const uint8_t* rgb_d,
                          const uint8_t* mask_d, const float E[16], void* stream);
/* As semtsdf_integrate_dev, with the frame prepass (pixel records, depth pyramid, unit
 * cull) on the volume's own prep stream, ordered only after inputs_ready (a hipEvent_t
 * marking the inputs complete; NULL: the inputs are already complete) and after the
 * integrate two frames back -- not after the earlier work of `stream` -- so it overlaps the
 * previous frame's integrate.  The integrate itself is ordered on `stream` as usual.  The
 * inputs must stay unchanged until this frame's integrate has run. */
int semtsdf_integrate_dev_async(semtsdf_vol* v, const uint16_t* depth_d, const uint8_t* rgb_d,
                                const uint8_t* mask_d, const float E[16], void* inputs_ready, void* stream);
/* Label-vote mode input (TSDF_Python/tsdf.cu:48-57): cls is int32 [H*W]. */
int semtsdf_integrate_vote_dev(semtsdf_vol* v, const uint16_t* depth_d, const uint8_t* rgb_d,
                               const int32_t* cls_d, const float E[16], void* stream);

/* ---- association (a5 + a6) -----------------------------------------------------------
 * Raycast the volume from the current camera (back_proj_kernel tsdf.cu:72-135), fuse the
 * 32x32 log-likelihood accumulation on device, decide assignments (tsdf.cu:337-389) and
 * relabel the mask in place.  Requires n_obs > 0 (tsdf.cu:426).  Host-pointer variant
 * copies the mask in and the relabelled mask back out; stats may be NULL. */
int semtsdf_associate(semtsdf_vol* v, uint8_t* mask_inout, const float E[16],
                      semtsdf_assoc_stats* stats, void* stream);
int semtsdf_associate_dev(semtsdf_vol* v, uint8_t* mask_d, const float E[16],
                          semtsdf_assoc_stats* stats_host_or_null, void* stream);
/* Debug/parity: per-pixel probs [H*W*32] f32 and box_mask [H*W*32] u8 exactly as the
 * reference back_proj_kernel leaves them (zeros where no hit).  Host outputs. */
int semtsdf_assoc_probs(semtsdf_vol* v, const float E[16], float* probs, uint8_t* box_mask, void* stream);
/* TSDF::filter_overlaps (tsdf.cu:304-416) on given inputs: probs_d f32 [H*W][32], box_d u8
 * [H*W][32] (nonzero = set), mask_d u8 [H*W] relabelled in place; n_obs, num_objs and the
 * knobs of the handle (n_obs > 0).  The decision the association march feeds, on the
 * reference's own function boundary (device pointers; async unless stats is given). */
int semtsdf_filter_overlaps_dev(semtsdf_vol* v, const float* probs_d, const uint8_t* box_d, uint8_t* mask_d,
                                semtsdf_assoc_stats* stats_host_or_null, void* stream);
/* The association's f32 logf (fn 0) / expf (fn 1) on the device over n values (device
 * pointers): the host C library's results bit for bit (semtsdf_libm.h), for verification;
 * fn 2: the device's own logf, which the march's fixed-point sums use (within the
 * certificate's slack of the host's). */
int semtsdf_libm_eval(int fn, const float* x_d, float* y_d, size_t n, void* stream);

/* ---- per-frame driver (a7: TSDF::parse_frame/launch_kernel tsdf.cu:171-228,418-504) ----
 * Integrated-frame count n_obs: if n_obs > 0 associate (relabels mask), else
 * num_objs = max(mask)+1; then integrate; n_obs++.  Placement is the caller's job
 * (semtsdf_place_from_frame + semtsdf_create). */
int semtsdf_parse_frame(semtsdf_vol* v, const uint16_t* depth, const uint8_t* rgb,
                        uint8_t* mask_inout, const float E[16], semtsdf_assoc_stats* stats, void* stream);
int semtsdf_parse_frame_dev(semtsdf_vol* v, const uint16_t* depth_d, const uint8_t* rgb_d,
                            uint8_t* mask_d, const float E[16], void* stream);
/* parse_frame_dev whose integrate (the frame's only write of the volume) first waits for
 * `integrate_after_event` (a hipEvent_t, or NULL), e.g. the end of the previous frame's live
 * render on another stream; the association, which only reads the volume, may overlap it. */
int semtsdf_parse_frame_dev_after(semtsdf_vol* v, const uint16_t* depth_d, const uint8_t* rgb_d,
                                  uint8_t* mask_d, const float E[16], void* integrate_after_event, void* stream);
/* parse_frame_dev plus one live view (semtsdf_raycast_dev arguments) of the volume as it
 * stands BEFORE this frame -- the view Viewer::show_tsdf shows after the previous frame
 * (kernel.cpp:96-107) -- rendered in the same launch as this frame's association march: both
 * read that state and both are bound by their slowest rays, so each fills the other's tail.
 * Without an association (first frame, non-semantic volume) the view is rendered first, alone.
 * out_bgr_d / out_t_d are written by the time the frame's work on `stream` completes. */
int semtsdf_parse_frame_view_dev(semtsdf_vol* v, const uint16_t* depth_d, const uint8_t* rgb_d,
                                 uint8_t* mask_d, const float E[16], const float s2w[16], const float c[3],
                                 int mode, uint8_t* out_bgr_d, float* out_t_d, void* stream);

/* ---- raycast render (a8: Viewer::show_tsdf viewer.cu:137-179) -------------------------
 * Orbit camera helper: s2w = rot(angle, dist) * Kinv, c = ((dist+0.5) sin, 0, (dist+0.5)(1-cos)). */
int semtsdf_orbit_camera(const float Kinv[16], float angle, float dist, float s2w[16], float c[3]);
/* out_bgr u8 [H*W*3] (host) black where nothing is hit; out_t f32 [H*W] (host, optional)
 * refined hit distance or -1. */
int semtsdf_raycast(semtsdf_vol* v, const float s2w[16], const float c[3], int mode,
                    uint8_t* out_bgr, float* out_t, void* stream);
int semtsdf_raycast_dev(semtsdf_vol* v, const float s2w[16], const float c[3], int mode,
                        uint8_t* out_bgr_d, float* out_t_d, void* stream);

/* ---- model maps of a view (no reference counterpart) --------------------------------------------
 * What the fused model shows along every ray of a view, read-only: hit distance, world position,
 * surface normal, instance id with its vote count, and a validity byte.  All arithmetic is f32,
 * every operation rounded on its own unless written fmaf; the view's width and height are the
 * handle's.  Per pixel (x, y):
 * Ray and hit: (o, d) as the raycast forms them: p = s2w (x, y, 1) + s2w[:,3] (dot3 then one add),
 *   r = p - c, d = r * (1 / sqrtf(dot3(r, r))), o = c.  t is the raycast's march and refinement, so
 *   t equals semtsdf_raycast's out_t bit for bit.  No hit: t = -1, flags = 0, every other output 0.
 * Point: P[a] = fmaf(t, d[a], o[a]); point = P.
 * Label and votes: the label render's rule at P without the palette: the trilinear histogram value
 *   of every bin (clamped sampler, mix(a, b, f) = fmaf(f, b, (1 - f) * a), x then y then z), the
 *   strict maximum over the bins in ascending order starting from max = 0.0f.  label = its bin
 *   (0: none), votes = max.
 * Normal: central differences of trilinear sdf samples one voxel apart.  For each axis a, P+ is P
 *   with component a replaced by P[a] + voxel[a] and P- by P[a] - voxel[a] (one add each); s+ and s-
 *   are the clamped trilinear sdf samples there; g[a] = (s+ - s-) / (voxel[a] + voxel[a]), an IEEE
 *   division.  n2 = dot3(g, g) = fmaf(g2, g2, fmaf(g1, g1, g0 * g0)), inv = 1.0f / sqrtf(n2),
 *   normal[a] = g[a] * inv.  The normal points from negative to positive sdf, into free space: the
 *   mesh's convention.
 * Validity: flags bit 0 (SEMTSDF_MAP_HIT) = hit.  Bit 1 (SEMTSDF_MAP_NORMAL) is set iff all 8
 *   corners of each of the six samples have weight >= min_weight (the 48 corner indices of the
 *   clamped sampler, clamped duplicates included) and n2 > 0.0f and n2 is finite.  Otherwise
 *   normal = (0, 0, 0).
 * Every pointer of semtsdf_maps_out may be NULL, and an output that is not requested costs nothing:
 * the histogram is sampled only for label or votes, the six sdf samples and the weights are read
 * only for normal or flags.  Errors, all decided before any device work: NULL v, s2w, c or out, or
 * all six pointers NULL: SEMTSDF_ERR_INVALID; a Z-sharded handle: SEMTSDF_ERR_UNSUPPORTED; label or
 * votes on a volume without SEMTSDF_F_SEMANTIC: SEMTSDF_ERR_STATE.  The launch counts as a render in
 * the timing (render_ms, n_render).  The volume is not modified; two calls on one state return
 * identical bytes.
 * semtsdf_render_maps: host buffers, synchronises; its device scratch (34 B per pixel) is kept on the
 *   handle after the first call; failing to get it is SEMTSDF_ERR_OOM and the handle stays usable.
 * semtsdf_render_maps_dev: device buffers, asynchronous on the stream.
 * semtsdf_pose_camera: the camera whose pixel grid is that of a frame fused with extrinsic E:
 *   Rt = E[:3,:3]^T, o = -Rt E[:3,3], s2w[:3,:3] = Rt Kinv[:3,:3], s2w[:3,3] = o, last row
 *   (0, 0, 0, 1), c = o; products and sums accumulated in double (ascending index) and rounded once
 *   to f32.  The raycast then forms r = (M p + o) - o, so its rays agree with the association's
 *   (Rt (Kinv p), no origin added and removed) only to about an ulp of |o|: they are not bit-equal. */
#define SEMTSDF_MAP_HIT 0x1u
#define SEMTSDF_MAP_NORMAL 0x2u
typedef struct semtsdf_maps_out { /* each pointer may be NULL; [H*W] or [H*W*3], row-major */
    float* t;
    float* point;
    float* normal;
    uint8_t* label;
    float* votes;
    uint8_t* flags;
} semtsdf_maps_out;
int semtsdf_render_maps(semtsdf_vol* v, const float s2w[16], const float c[3], int32_t min_weight,
                        const semtsdf_maps_out* out_host, void* stream);
int semtsdf_render_maps_dev(semtsdf_vol* v, const float s2w[16], const float c[3], int32_t min_weight,
                            const semtsdf_maps_out* out_dev, void* stream);
int semtsdf_pose_camera(const float Kinv[16], const float E[16], float s2w[16], float c[3]);

/* ---- camera tracking: frame maps and the point-to-plane system (no reference counterpart) --------
 * What one iteration of frame-to-model ICP needs from the device: the camera-space vertex and normal
 * of every depth pixel (the frame-side counterpart of the model maps), and the normal equations of
 * the point-to-plane error between those and the model maps of a reference view, as order-free
 * fixed-point sums.  The 6 x 6 solve and the pose update are the host's (semtsdf/track.py).  All
 * arithmetic is f32, every operation rounded on its own, with dot3(a, b) = fmaf(a2, b2, fmaf(a1, b1,
 * a0 * b0)) as in the model maps and cross(a, b) = (a1 * b2 - a2 * b1, a2 * b0 - a0 * b2, a0 * b1 -
 * a1 * b0): two rounded products and one subtraction per component, no fmaf.  Width W, height H, K,
 * Kinv and depth_scale are the handle's; neither call reads or modifies the volume.
 *
 * Frame maps.  Per pixel (x, y) with raw depth D (u16):
 * Vertex: z = (float)D / depth_scale (an IEEE division: the value the integrate's pixel record
 *   holds), r[a] = dot3(Kinv[a][0..2], ((float)x, (float)y, 1.0f)), V[a] = r[a] * z.  flags bit 0 =
 *   (D != 0); where D == 0, V = (+0, +0, +0).
 * Normal: A = V(x, y + 1) - V, B = V(x + 1, y) - V (componentwise), g = cross(A, B), n2 = dot3(g, g),
 *   inv = 1.0f / sqrtf(n2), n[a] = g[a] * inv.  It points towards the camera, into free space: the
 *   model maps' convention.  flags bit 1 is set iff x + 1 < W and y + 1 < H, the three depths are
 *   nonzero, n2 > 0.0f and n2 is finite; otherwise n = (+0, +0, +0).
 * No smoothing and no pyramid: the gates below reject depth edges.  Every output pointer may be NULL
 * (all three NULL: SEMTSDF_ERR_INVALID); an output requested alone equals that of the full call.
 * semtsdf_frame_maps: host buffers, synchronises.  semtsdf_frame_maps_dev: device buffers,
 * asynchronous on the stream.
 *
 * The system of one iteration.  Inputs (semtsdf_icp_in): the frame maps above and the model maps
 * point, normal, flags of a reference view as semtsdf_render_maps wrote them for
 * semtsdf_pose_camera(Kinv, E_ref); E_ref; E_cur, the current estimate (volume to camera, the
 * integrate's convention); dist_max (metres), cos_min, stride.  On the host, before the launch:
 *   Rt = E_cur[:3,:3]^T and o = -Rt E_cur[:3,3] exactly as semtsdf_pose_camera forms them (sums of
 *   double products in ascending index, rounded once to f32); dmax2 = dist_max * dist_max (one f32
 *   product).
 * Every frame pixel (x, y) with x % stride == 0, y % stride == 0 and frame flags & 3 == 3 is visited
 * and falls into exactly one of four classes, by these steps in order (V, n: its frame maps):
 *  1. Pw[a] = dot3(Rt[a], V) + o[a];  Nw[a] = dot3(Rt[a], n).
 *  2. q[a] = dot3(E_ref[a][0..2], Pw) + E_ref[a][3];  s[a] = dot3(K[a][0..2], q).  Class none if
 *     q[2] <= 0.  u = floorf(s[0] / s[2] + 0.5f), v = floorf(s[1] / s[2] + 0.5f) (IEEE divisions).
 *     Class none unless 0 <= u < W and 0 <= v < H (compared as floats, so a NaN is off the image) and
 *     the model flags at (u, v) have both SEMTSDF_MAP_HIT and SEMTSDF_MAP_NORMAL.  Pm, Nm: the model
 *     point and normal at (u, v).
 *  3. d[a] = Pm[a] - Pw[a].  Class far if dot3(d, d) > dmax2.
 *  4. Class angle if dot3(Nm, Nw) < cos_min.
 *  5. r = dot3(Nm, d);  J = (cross(Pw, Nm), Nm), six values.  Class none unless every |J[i]| < 32 (a
 *     NaN is out of range): the range gate that bounds the sums below.
 *  6. Inlier.  Each product J[i] * J[j] (i <= j), J[i] * r and r * r is formed in double (exact for f32
 *     factors), multiplied by 2^32 (exact), rounded to nearest-even to int64 and added to its word.
 * Output: 32 int64 words.  0..20: the upper triangle of J^T J, row-major ((0,0), (0,1), .. (0,5),
 * (1,1), .. (5,5)); 21..26: J^T r; 27: sum of r^2; 28: inliers; 29: far; 30: angle; 31: none.  Words
 * 28..31 are plain counts and sum to the number of pixels visited.  The rows describe the twist
 * xi = (omega, v) of the volume frame that minimises sum (r - J xi)^2: solve (J^T J) xi = J^T r and
 * move the camera by C2W <- exp(xi) C2W.  Each term is below 2^10 * 2^32 = 2^42 in magnitude and
 * W * H <= 2^19, so no sum reaches 2^61; integer sums do not depend on order, so the words are the
 * same on every run and for every reduction shape.
 * Errors, all decided before any device work: a NULL argument or input pointer, W * H > 2^19,
 * stride < 1, dist_max outside (0, 1] or cos_min outside [-1, 1] (a NaN is outside):
 * SEMTSDF_ERR_INVALID; a Z-sharded handle: SEMTSDF_ERR_UNSUPPORTED (both calls, as for the maps).
 * semtsdf_icp_system_dev: device pointers in `in_dev` and `words_dev`; zeroes the words on the
 *   stream, then one launch; asynchronous, nothing is read back.
 * semtsdf_icp_system: host pointers; uploads the six maps, runs the same launch and synchronises.
 * The host variants keep their device scratch (52 B per pixel) on the handle after the first call. */
typedef struct semtsdf_icp_in { /* [H*W] or [H*W*3], row-major */
    const float* vertex;     /* frame maps */
    const float* normal;
    const uint8_t* flags;
    const float* m_point;    /* model maps of the reference view */
    const float* m_normal;
    const uint8_t* m_flags;
} semtsdf_icp_in;
#define SEMTSDF_ICP_WORDS 32
int semtsdf_frame_maps(semtsdf_vol* v, const uint16_t* depth, float* vertex, float* normal, uint8_t* flags,
                       void* stream);
int semtsdf_frame_maps_dev(semtsdf_vol* v, const uint16_t* depth_d, float* vertex_d, float* normal_d,
                           uint8_t* flags_d, void* stream);
int semtsdf_icp_system(semtsdf_vol* v, const semtsdf_icp_in* in_host, const float E_ref[16], const float E_cur[16],
                       float dist_max, float cos_min, int32_t stride, int64_t* words_host, void* stream);
int semtsdf_icp_system_dev(semtsdf_vol* v, const semtsdf_icp_in* in_dev, const float E_ref[16],
                           const float E_cur[16], float dist_max, float cos_min, int32_t stride, int64_t* words_dev,
                           void* stream);

/* ---- depth pyramid: coarse-to-fine tracking on filtered depth (no reference counterpart) -----------
 * The frame side of coarse-to-fine ICP: an edge-preserving filter of the depth image (level 0), up to
 * three band-limited halvings of it, the frame maps of every level, and the system of one iteration
 * with a frame grid of its own.  All arithmetic is f32 and every operation is rounded on its own
 * unless written fmaf; there is no exp, the weights are polynomials.  W, H, K, Kinv and depth_scale are
 * the handle's; no call reads or modifies the volume.
 *
 * Level geometry.  Level 0 is W x H with Kinv the upper-left 3 x 3 of the handle's Kinv, copied as
 * it is.  Level l has width W >> l and height H >> l (floor).  With fx = K[0], fy = K[5], cx = K[2],
 * cy = K[6], its camera is formed in double: fx_l = fx / 2^l, fy_l = fy / 2^l, cx_l = (cx + 0.5) / 2^l -
 * 0.5, cy_l likewise (pixel centres lie at integers; coarse pixel x covers the fine pixels 2x and
 * 2x + 1), and Kinv_l = [[1 / fx_l, 0, -cx_l / fx_l], [0, 1 / fy_l, -cy_l / fy_l], [0, 0, 1]], each entry
 * rounded once to f32.
 *
 * Level 0 depth.  zc = (float)D / depth_scale of raw depth D (the frame maps' value).  radius 0:
 * z0 = zc.  radius R in 1..4: D == 0 gives z0 = +0 (holes are never filled).  Otherwise, with
 * inv_s = 1.0f / (float)((R + 1)^2) and inv_r = 1.0f / sigma_r (IEEE divisions, formed before the
 * launch), num = den = 0 and the neighbours (x + dx, y + dy) visited with dy = -R..R ascending, then
 * dx = -R..R ascending: a neighbour off the image or with raw depth 0 is skipped; so is one with
 * us = 1.0f - (float)(dx^2 + dy^2) * inv_s not > 0 (at R = 4 that leaves 69 of the 81 taps, at R = 3 45
 * of 49); for the rest, zn the neighbour's (float)D / depth_scale: d = zn - zc, e = d * inv_r,
 * u = 1.0f - e * e, skipped unless u > 0; w = (us * us) * (u * u) (three rounded products),
 * num = fmaf(w, d, num), den = den + w.  z0 = zc + num / den (an IEEE division; the centre contributes
 * w = 1, so den >= 1).  A neighbour further than sigma_r in depth has no weight, so a step larger than
 * sigma_r is left exactly as it is, and a constant image comes back bit for bit.
 *
 * Halving.  Level l + 1 at (x, y), with b = z_l(2x, 2y): b == 0 gives +0.  Otherwise s = n = 0 and for
 * q = z_l(2x, 2y), z_l(2x + 1, 2y), z_l(2x, 2y + 1), z_l(2x + 1, 2y + 1) in that order, each with q != 0 and
 * fabsf(q - b) <= band: s = s + (q - b), n = n + 1.  z_{l+1} = b + s / (float)n.
 *
 * Maps of a level: the frame maps' rule (above) with the level's z in place of (float)D / depth_scale
 * and the level's Kinv, width and height; flags bit 0 = (z != 0).  With radius 0, level 0 equals
 * semtsdf_frame_maps in every bit.
 *
 * semtsdf_frame_level: width, height and Kinv are written by the library; z is required at every level,
 * vertex, normal and flags may each be NULL; an output requested alone equals that of the full call.
 * semtsdf_frame_levels: writes width, height and Kinv of nlevels levels and touches no device.
 * semtsdf_frame_pyramid_dev: device pointers (depth_d and those in the structs, which stay host
 *   memory); allocates nothing, only enqueues on the stream (the filter, nlevels - 1 halvings, one maps
 *   launch per level with an output), reads nothing back.
 * semtsdf_frame_pyramid: host pointers; synchronises.  Its device scratch (2 B per pixel and 29 B per
 *   pixel of each of the four levels the image admits) is the handle's, counted in device_bytes and
 *   kept after the first call; failing to get it is SEMTSDF_ERR_OOM and the handle stays usable.
 * Errors, all decided before any device work: a NULL argument or a NULL z; nlevels outside
 * 1..SEMTSDF_PYRAMID_MAX_LEVELS; a coarsest level narrower or lower than 2 pixels; nlevels > 1 with K[1]
 * or K[4] nonzero; radius outside 0..4; radius > 0 with sigma_r not finite or <= 0; nlevels > 1 with
 * band not finite or <= 0: SEMTSDF_ERR_INVALID.  A Z-sharded handle: SEMTSDF_ERR_UNSUPPORTED.
 *
 * semtsdf_icp_system_level: semtsdf_icp_system with two pixel grids.  The visited pixels, stride and
 * the row pitch of the frame maps come from frame_width x frame_height; Pw is projected, bounded and
 * looked up in the model maps with the handle's K, W and H: the model maps stay the one
 * full-resolution render of the reference view, and a coarse frame pixel finds a true model point
 * and normal, which is all that projective association asks for.  Steps, words and errors are
 * semtsdf_icp_system's, with frame_width, frame_height >= 1 and frame_width * frame_height <= 2^19 in
 * place of its bound on W * H (the host variant also needs frame_width * frame_height <= W * H: it
 * shares semtsdf_icp_system's scratch).  With frame_width = W and frame_height = H the words are
 * semtsdf_icp_system's. */
#define SEMTSDF_PYRAMID_MAX_LEVELS 4
typedef struct semtsdf_frame_level {
    int32_t width, height; /* written by the library */
    float Kinv[9];         /* written: row-major 3x3 of the level */
    float* z;              /* [h*w] metres, 0 = no depth; required at every level */
    float* vertex;         /* [h*w*3] optional */
    float* normal;         /* [h*w*3] optional */
    uint8_t* flags;        /* [h*w]   optional */
} semtsdf_frame_level;
int semtsdf_frame_levels(const semtsdf_vol* v, int nlevels, semtsdf_frame_level* levels);
int semtsdf_frame_pyramid(semtsdf_vol* v, const uint16_t* depth, int radius, float sigma_r, float band, int nlevels,
                          semtsdf_frame_level* levels_host, void* stream);
int semtsdf_frame_pyramid_dev(semtsdf_vol* v, const uint16_t* depth_d, int radius, float sigma_r, float band,
                              int nlevels, semtsdf_frame_level* levels_dev, void* stream);
int semtsdf_icp_system_level(semtsdf_vol* v, const semtsdf_icp_in* in_host, int32_t frame_width, int32_t frame_height,
                             const float E_ref[16], const float E_cur[16], float dist_max, float cos_min,
                             int32_t stride, int64_t* words_host, void* stream);
int semtsdf_icp_system_level_dev(semtsdf_vol* v, const semtsdf_icp_in* in_dev, int32_t frame_width,
                                 int32_t frame_height, const float E_ref[16], const float E_cur[16], float dist_max,
                                 float cos_min, int32_t stride, int64_t* words_dev, void* stream);

/* ---- RGB-D tracking: a photometric term beside point-to-plane ICP (no reference counterpart) --------
 * Point-to-plane ICP has no constraint along a plane or around its normal.  A dense photometric term
 * between the frame's colour image and the colour render of the model (semtsdf_raycast,
 * SEMTSDF_RENDER_COLOR, at semtsdf_pose_camera(Kinv, E_ref): the view of the model maps, same t) adds
 * one.  Two calls: the intensity pyramid of a colour image, and the system of one iteration with both
 * terms, 64 words from one launch.  W, H, K are the handle's; no call reads or modifies the volume.
 *
 * Intensity pyramid.  Input: a u8 x 3 image [H*W*3], an optional u8 validity image [H*W] (nonzero =
 * valid, NULL = all valid), nlevels in 1..SEMTSDF_PYRAMID_MAX_LEVELS.  Level l is (W >> l) x (H >> l),
 * the depth pyramid's sizes.  Everything is an integer until one exact conversion:
 *   Y = c0 + 2 c1 + c2 of the three channels (symmetric in the outer two: RGB and BGR images agree).
 *   S_0(x, y) = sum over dy, dx in -1..1 of b(dy) b(dx) Y(clamp(x + dx, 0, W - 1), clamp(y + dy, 0, H - 1))
 *     with b = (1, 2, 1): at most 16 * 1020 = 16320.  valid_0(x, y) = 1 iff all nine clamped taps are
 *     valid, else 0.
 *   S_{l+1}(x, y) = S_l(2x, 2y) + S_l(2x + 1, 2y) + S_l(2x, 2y + 1) + S_l(2x + 1, 2y + 1);  valid_{l+1} = 1
 *     iff all four are valid.
 *   The intensity of a pixel of level l is I = (float)S_l * 2^-(14 + 2l), exact and in [0, 1).
 * semtsdf_intensity_level: width and height are written by the library; S (u32) and valid (u8) are
 * both required at every level.  One launch builds all levels.
 * semtsdf_intensity_pyramid_dev: device pointers (rgb_d, valid_d and those in the structs, which stay
 *   host memory); allocates nothing, one launch on the stream, reads nothing back.
 * semtsdf_intensity_pyramid: host pointers; synchronises.  Its device scratch (4 B per pixel, 5 B per
 *   pixel of each of the four levels the image admits, and 10 B per pixel with 512 B for the host
 *   variant of the system below) is the handle's, counted in device_bytes and kept after the first
 *   call; failing to get it is SEMTSDF_ERR_OOM and the handle stays usable.
 * Errors, all decided before any device work: a NULL argument other than valid, a NULL S or valid of
 * a level, nlevels outside 1..SEMTSDF_PYRAMID_MAX_LEVELS, a coarsest level narrower or lower than 2
 * pixels: SEMTSDF_ERR_INVALID.  A Z-sharded handle: SEMTSDF_ERR_UNSUPPORTED.
 *
 * The RGB-D system of one iteration, on pyramid level l.  Inputs: semtsdf_icp_in with the frame maps
 * of level l of the depth pyramid ((W >> l) x (H >> l); level 0 may be semtsdf_frame_maps') and the
 * full-resolution model maps of the reference view, as for semtsdf_icp_system_level; semtsdf_rgbd_in:
 * S_l and valid_l of the frame's colour image and of the model's colour render, the latter built with
 * the validity (m_flags & 3) == 3 (SEMTSDF_MAP_NORMAL says that the eight corners of the colour sample
 * were observed); r_max, the gate on the intensity residual.  On the host, before the launch: Rt, o,
 * dmax2 as for semtsdf_icp_system; the level camera as semtsdf_frame_levels forms it, in double,
 * rounded once to f32: fx_l = K[0] / 2^l, fy_l = K[5] / 2^l, cx_l = (K[2] + 0.5) / 2^l - 0.5, cy_l likewise.
 * w_l = W >> l, h_l = H >> l.
 * Words 0..31 are semtsdf_icp_system_level's on the same inputs with frame_width = w_l and
 * frame_height = h_l, by its rule, untouched.
 * Words 32..63 are the photometric system in the same layout (21 upper-triangle words, 6 of J^T r, the
 * sum of r^2, then the counts of inliers, far, outlier, none).  Every frame pixel (x, y) on the stride
 * with frame flags bit 0 set and the frame's valid_l set is visited and falls into exactly one class,
 * by these steps in order.  All arithmetic is f32, every operation rounded on its own unless written
 * fmaf; dot3 and cross are those of the camera tracking section.
 *  1. Pw as step 1 of semtsdf_icp_system.
 *  2. q, s, u, v as its step 2 (the full-resolution projection).  Class none if q[2] <= 0, if (u, v) is
 *     off the image (not 0 <= u < W and 0 <= v < H, compared as floats) or if the model flags at (u, v)
 *     lack SEMTSDF_MAP_HIT.  Pm: the model point there.
 *  3. d[a] = Pm[a] - Pw[a].  Class far if dot3(d, d) > dmax2: the occlusion gate.
 *  4. iz = 1.0f / q[2];  ul = fmaf(fx_l, q[0] * iz, cx_l), vl = fmaf(fy_l, q[1] * iz, cy_l);  x0 =
 *     floorf(ul), y0 = floorf(vl).  Class none unless 0 <= x0, x0 + 1 < w_l, 0 <= y0, y0 + 1 < h_l
 *     (compared as floats) and the model's valid_l is set at (x0, y0), (x0 + 1, y0), (x0, y0 + 1),
 *     (x0 + 1, y0 + 1).  ax = ul - x0, ay = vl - y0.
 *  5. With m00, m10, m01, m11 the model's intensities at those four taps: dx0 = m10 - m00,
 *     dx1 = m11 - m01, top = fmaf(ax, dx0, m00), bot = fmaf(ax, dx1, m01), Im = fmaf(ay, bot - top, top);
 *     the exact gradient of that bilinear patch: gx = fmaf(ay, dx1 - dx0, dx0),
 *     gy = fmaf(ax, (m11 - m10) - (m01 - m00), m01 - m00).
 *  6. r = If - Im with If the frame's intensity at (x, y).  Class outlier if fabsf(r) > r_max.
 *  7. a0 = (gx * fx_l) * iz, a1 = (gy * fy_l) * iz, a2 = -((a0 * q[0] + a1 * q[1]) * iz): the gradient of
 *     Im by q.  aw[k] = dot3((E_ref[0][k], E_ref[1][k], E_ref[2][k]), (a0, a1, a2)): by Pw.
 *     J = (cross(Pw, aw), aw).  Class none unless every |J[i]| < 2048 (a NaN is out of range).
 *  8. Inlier.  Each product J[i] * J[j] (i <= j), J[i] * r and r * r is formed in double, multiplied by
 *     2^20, rounded to nearest-even to int64 and added to its word.
 * C2W <- exp(xi) C2W moves Pw by omega x Pw + v, so Im changes by J . xi to first order and r - J xi is
 * the residual after the step: the normal equations and the sign are the point-to-plane system's, and
 * the two add as (A_g + w^2 A_p) xi = b_g + w^2 b_p for a weight w in metres per unit of intensity.
 * Each term is below 2^22 * 2^20 = 2^42 and at most 2^19 pixels are visited, so no sum reaches 2^61.
 * Errors, all decided before any device work: those of semtsdf_icp_system_level; a NULL rgbd_in or
 * intensity pointer; level outside 0..SEMTSDF_PYRAMID_MAX_LEVELS - 1, or with W >> level or H >> level
 * below 2; K[1] or K[4] nonzero (the level camera has no skew); r_max outside (0, 1] (a NaN is
 * outside): SEMTSDF_ERR_INVALID.  A Z-sharded handle: SEMTSDF_ERR_UNSUPPORTED.
 * semtsdf_rgbd_system_level_dev: device pointers; zeroes the 64 words on the stream, then one launch;
 *   asynchronous, nothing is read back.
 * semtsdf_rgbd_system_level: host pointers; uploads the maps and the four intensity arrays, runs the
 *   same launch and synchronises.  It shares semtsdf_icp_system's scratch and the intensity pyramid's. */
typedef struct semtsdf_intensity_level {
    int32_t width, height; /* written by the library */
    uint32_t* S;           /* [h*w] required */
    uint8_t* valid;        /* [h*w] required */
} semtsdf_intensity_level;
typedef struct semtsdf_rgbd_in { /* level l: [(H >> l) * (W >> l)] */
    const uint32_t* f_S;     /* the frame's colour image */
    const uint8_t* f_valid;
    const uint32_t* m_S;     /* the model's colour render at the reference view */
    const uint8_t* m_valid;
} semtsdf_rgbd_in;
#define SEMTSDF_RGBD_WORDS 64
int semtsdf_intensity_pyramid(semtsdf_vol* v, const uint8_t* rgb, const uint8_t* valid, int nlevels,
                              semtsdf_intensity_level* levels_host, void* stream);
int semtsdf_intensity_pyramid_dev(semtsdf_vol* v, const uint8_t* rgb_d, const uint8_t* valid_d, int nlevels,
                                  semtsdf_intensity_level* levels_dev, void* stream);
int semtsdf_rgbd_system_level(semtsdf_vol* v, const semtsdf_icp_in* in_host, const semtsdf_rgbd_in* photo_host,
                              int32_t level, const float E_ref[16], const float E_cur[16], float dist_max,
                              float cos_min, float r_max, int32_t stride, int64_t* words_host, void* stream);
int semtsdf_rgbd_system_level_dev(semtsdf_vol* v, const semtsdf_icp_in* in_dev, const semtsdf_rgbd_in* photo_dev,
                                  int32_t level, const float E_ref[16], const float E_cur[16], float dist_max,
                                  float cos_min, float r_max, int32_t stride, int64_t* words_dev, void* stream);

/* ---- Z-sharded raycast (replaces the single-GPU back_proj_kernel
 * tsdf.cu:72-135 and show_tsdf_kernel viewer.cu:17-86 when the volume is split across GPUs)
 * Every shard of a group runs the same call sequence.  Between calls the host exchanges
 * the per-pixel `send` records (record_bytes each) of all shards into `gathered` (device
 * memory) as `exchange` says (SEMTSDF_EXCHANGE_*):
 *   begin(kind, cam, c, exchange, &rec, &nsteps)
 *   for s in 0..nsteps-1:  step(s, s ? gathered : NULL, send);  all-gather send -> gathered
 *   kind RENDER_*:  render_finish(gathered, out_bgr, out_t)   -- all-gathered composite
 *   kind RAY_ASSOC: assoc_partial(gathered, mask, partial);    all-reduce(SUM) partial;
 *                   assoc_apply(reduced, mask, stats)         -- decide + relabel
 * The result is bit-identical to the single-volume raycast / association. */
#define SEMTSDF_RAY_ASSOC 2
#define SEMTSDF_ASSOC_PARTIAL_LEN 3168 /* int64 words: 32x32 t1, t3; 32 t2, c1, c2; 32x32 c3
                                         (the unused c1[0] word: the largest positive term) */
/* exchange between protocol steps: every shard's records concatenated in shard order
 * (all-gather; gathered = z_nshards * record_bytes), or their element-wise minimum as
 * little-endian int64 (all-reduce MIN; gathered = record_bytes), 1/z_nshards of the bytes. */
#define SEMTSDF_EXCHANGE_ALLGATHER 0
#define SEMTSDF_EXCHANGE_MIN 1
int semtsdf_shard_ray_begin(semtsdf_vol* v, int kind, const float cam[16], const float c[3], int exchange,
                            size_t* record_bytes, int* nsteps);
int semtsdf_shard_ray_step(semtsdf_vol* v, int step, const void* gathered_d, void* send_d, void* stream);
int semtsdf_shard_render_finish(semtsdf_vol* v, const void* gathered_d, uint8_t* out_bgr_d, float* out_t_d,
                                void* stream);
int semtsdf_shard_assoc_partial(semtsdf_vol* v, const void* gathered_d, const uint8_t* mask_d,
                                int64_t* partial_d, void* stream);
int semtsdf_shard_assoc_apply(semtsdf_vol* v, const int64_t* reduced_d, uint8_t* mask_d,
                              semtsdf_assoc_stats* stats, void* stream);
/* When assoc_apply returns SEMTSDF_NEED_PIXELS (some labels are too close to call from the
 * reduced fixed-point sums; nothing was decided or relabelled):
 *   assoc_pixels(gathered, px): this shard's per-pixel association data, zeros for pixels it
 *       does not own; all-reduce(SUM, int32) px over the group;
 *   assoc_apply_exact(reduced, px_reduced, mask, stats): decide + relabel.
 * px: SEMTSDF_ASSOC_PIXEL_WORDS int32 words per pixel (device memory). */
#define SEMTSDF_ASSOC_PIXEL_WORDS 34
int semtsdf_shard_assoc_pixels(semtsdf_vol* v, const void* gathered_d, int32_t* px_d, void* stream);
int semtsdf_shard_assoc_apply_exact(semtsdf_vol* v, const int64_t* reduced_d, const int32_t* px_d, uint8_t* mask_d,
                                    semtsdf_assoc_stats* stats, void* stream);
/* dst[i] = min(dst[i], src[i]) over n int64 (device, async on stream): the exchange
 * SEMTSDF_EXCHANGE_MIN for shards driven from one process. */
int semtsdf_min_i64(int64_t* dst_d, const int64_t* src_d, size_t n, void* stream);
/* parse_frame for a sharded handle: the host runs the association protocol above (when
 * n_obs > 0), then integrate_dev (which advances n_obs and sets the first frame's object count).
 * note_integrated did that up to ABI 11; it is kept as a no-op that checks its handle. */
int semtsdf_shard_note_integrated(semtsdf_vol* v, const uint8_t* mask_d, void* stream);

/* ---- mask producer contract --------------------------------------
 * Detector output -> the u8 instance-label mask the fusion consumes, as Mask_RCNN/dmask.py's
 * mask_detect (dmask.py:47-59, without the optional depth filter that mask_process.py does
 * not use): detection i is kept when its area > min_area (filter_tiny_objects, 2000 in the
 * reference), a pixel belongs to the smallest kept detection containing it (preserve_small_objs;
 * equal areas: the lower index), labelled 1 + its index among the kept ones.
 * masks_d: bytes [height][width][n] (nonzero = inside; the detector's masks[H, W, N]),
 * labels_d: u8 [height * width]; 0 <= n <= 256; device pointers, async on stream.
 * n_kept (optional, host) receives the number of kept detections (synchronises). */
int semtsdf_masks_to_labels(const uint8_t* masks_d, int width, int height, int n, int min_area,
                            uint8_t* labels_d, int* n_kept, void* stream);

/* The same labels straight from the detector's pixel boxes and mini-masks, without the [height][width][n]
 * masks: detection i's mask is unmold_mask's (mrcnn/utils.py:565-581: skimage.transform.resize order=1
 * mode="constant" of the mini-mask to the box, without anti-aliasing as in the reference's era, then
 * >= 0.5), evaluated per pixel by the rule below; keep, rank and label are exactly those of
 * semtsdf_masks_to_labels (area > min_area; the smallest kept detection that is on at the pixel; equal
 * areas: the lower index; label 1 + index among the kept, wrapping as u8).
 *   boxes_d: [n][4] int32 pixel boxes (y1, x1, y2, x2), half-open, as unmold_detections / denorm_boxes
 *            leave them.  y2 <= y1 or x2 <= x1: an empty detection (area 0).  A box may reach outside the
 *            image; only the pixels inside both the box and the image exist.
 *   mini_d:  [n][mh][mw], each detection's own mask (its class already selected); dtype 0 fp16, 1 bf16,
 *            2 f32, every element converted to f32 exactly; 1 <= mh, mw <= 64
 *   0 <= n <= 256; width, height as semtsdf_masks_to_labels
 *   labels_d: u8 [height * width], every pixel written (n == 0: all zero)
 *   areas_d: u32 [n] or NULL: the number of `on` pixels of each detection
 *   work_d:  semtsdf_detections_to_labels_workspace(n) bytes of device memory
 *   n_kept:  optional, host: the number of kept detections (synchronises)
 * The rule, every operation rounded to f32 on its own (no fused multiply-add), for detection i with
 * h = y2 - y1, w = x2 - x1 and image pixel (y, x), max(y1, 0) <= y < min(y2, height) (likewise x):
 *   sy = (float)mh / (float)h;                   sx = (float)mw / (float)w
 *   cy = ((float)(y - y1) + 0.5f) * sy - 0.5f;   cx likewise
 *   y0 = floorf(cy), fy = cy - y0, taps iy = (int)y0 and iy + 1 (x likewise); a tap outside
 *   [0, mh) x [0, mw) reads 0.0f
 *   top = m[iy][ix] * (1.0f - fx) + m[iy][ix+1] * fx;  bot = m[iy+1][ix] * (1.0f - fx) + m[iy+1][ix+1] * fx
 *   v = top * (1.0f - fy) + bot * fy;  on = v >= 0.5f (a NaN is off)
 * The call allocates nothing and enqueues kernels only on stream (it can be recorded in a captured HIP
 * graph); it is asynchronous unless n_kept is given.  Argument errors return
 * SEMTSDF_ERR_INVALID before any device work.  Deterministic: integer sums, one writer per pixel. */
size_t semtsdf_detections_to_labels_workspace(int n);
int semtsdf_detections_to_labels(const int32_t* boxes_d, const void* mini_d, int dtype, int mh, int mw,
                                 int n, int width, int height, int min_area, uint8_t* labels_d,
                                 uint32_t* areas_d /* [n] or NULL */, void* work_d,
                                 int* n_kept /* host, optional: synchronises */, void* stream);

/* Achievable HBM bandwidth on `device` (GB/s, read + write bytes) of a float4 device copy
 * of `bytes` bytes, best of `reps` runs: the practical ceiling beside the 8 TB/s spec peak. */
int semtsdf_copy_bandwidth(int device, size_t bytes, int reps, double* gbs);

/* ---- state transfer (parity, checkpoint/resume) ------------------------------------------
 * Reference layouts, local storage (for an unsharded handle: the whole volume).  Any
 * pointer may be NULL.  color is u8 [N*3] or i32 [N*3] per SEMTSDF_F_COLOR_I32; hist is
 * voxel-major u32 [N*32] (tsdf.cu:249); cls/cls_cnt i32 [N] (vote mode). */
int semtsdf_download(semtsdf_vol* v, float* sdf, int32_t* wt, void* color, uint32_t* hist,
                     int32_t* cls, int32_t* cls_cnt);
/* The x-planes [x0, x1) only, same layouts (arrays sized (x1-x0) * Dy * local Dz [* 3 | * 32]):
 * checks of volumes too large to download whole (a 1024^3 histogram is 128 GiB). */
int semtsdf_download_slab(semtsdf_vol* v, int x0, int x1, float* sdf, int32_t* wt, void* color,
                          uint32_t* hist, int32_t* cls, int32_t* cls_cnt);
int semtsdf_upload(semtsdf_vol* v, const float* sdf, const int32_t* wt, const void* color,
                   const uint32_t* hist, const int32_t* cls, const int32_t* cls_cnt);

/* ---- surface export (no reference counterpart) -------------------------
 * Every stored voxel of this handle (a shard: its owned planes) with weight >= min_weight and
 * |sdf| < sdf_max (sdf in the volume's normalised units, f = diff / mu), in the reference's flat
 * order (x-major, z fastest; global indices), with its colour (int32 colours clamped to [0, 255])
 * and instance label (the argmax of its histogram, first maximum; 0 without a count).  out may
 * be NULL (count only); otherwise it receives min(count, capacity) points.  Synchronises. */
typedef struct semtsdf_surface_point {
    uint32_t x, y, z; /* voxel index; position = vol_start + index * voxel (tsdf.cu:30) */
    float sdf;
    uint8_t r, g, b, label;
} semtsdf_surface_point;
int semtsdf_export_surface(semtsdf_vol* v, float sdf_max, int32_t min_weight, semtsdf_surface_point* out,
                           uint64_t capacity, uint64_t* count);

/* ---- mesh extraction (no reference counterpart) ----------------------------------------------
 * The labelled triangle mesh of the sdf = 0 level set: marching tetrahedra on the Kuhn split.
 * Cells: the cube with min corner (x, y, z), 0 <= x < Dx-1, 0 <= y < Dy-1, 0 <= z < Dz-1 (global
 *   z), is valid iff all 8 corners have weight >= min_weight.  A corner is negative iff sdf < 0.0f
 *   (+0.0 and -0.0 are not).
 * Tetrahedra: 6 per cell, one per axis permutation (a, b, c), indexed by its lexicographic rank
 *   (xyz, xzy, yxz, yzx, zxy, zyx): v0 = the corner, v1 = v0 + e_a, v2 = v1 + e_b, v3 = v2 + e_c.
 * Edges, vertices: a tet edge (vi, vj), i < j, is named by its owner voxel vi and its class
 *   dx | dy << 1 | dz << 2 (1..7) of the offset vj - vi.  There is one mesh vertex per edge that an
 *   emitted triangle references, shared by all triangles using it.
 * Triangles of a tet with k negative vertices: none for k = 0, 4; for k = 1, 3 one on the three
 *   edges at the lone vertex; for k = 2, negatives A < B and others C < D in tet vertex order,
 *   (AC, AD, BD) and (AC, BD, BC).  Each is wound so that, with every crossing at its edge midpoint
 *   in index space, the right-hand normal points from the negative towards the non-negative
 *   vertices (into free space).  Degenerate triangles (a crossing on a voxel) are kept.
 * Position: s0 the owner's sdf, s1 the other endpoint's; t = s0 / (s0 - s1); per axis a,
 *   g = (float)index[a] + (d[a] ? t : 0.0f), pos[a] = g * voxel[a] + vol_start[a]: f32, one rounding
 *   per operation, a multiply then an add (not the fmaf of the voxel position rule tsdf.cu:30,
 *   from which it differs by at most 1 ulp at t = 0).
 * Attributes: colour (int32 colours clamped to [0, 255]) and label (histogram argmax, first
 *   maximum; 0 without a count or in a volume that is not SEMANTIC) of the endpoint nearer the
 *   surface: the owner if |s0| <= |s1|, else the other one.
 * Outputs are host pointers; the call synchronises.  verts == NULL && tris == NULL: count only
 * (one NULL alone is SEMTSDF_ERR_INVALID).  With both given and a capacity short:
 * SEMTSDF_ERR_INVALID, the counts written, the buffers untouched.  2^32 vertices or more:
 * SEMTSDF_ERR_UNSUPPORTED.  Scratch (29 B per 256 stored voxels to count, 4 B per stored voxel
 * more to emit, and the outputs) lives for the call; failing to get it is SEMTSDF_ERR_OOM and the
 * handle stays usable.  The volume is not modified.  The output is deterministic: two calls on
 * one state return identical bytes; the order is otherwise unspecified (canonical: vertices by
 * (x, y, z, edge)).  A shard extracts the cells whose min-corner plane it owns (keys carry the
 * global z), so the vertices on a chunk's halo plane appear in both neighbouring shards with
 * identical bytes; welding equal keys joins the shards' meshes into the whole volume's. */
typedef struct semtsdf_mesh_vertex { /* 32 bytes */
    float pos[3];
    uint32_t x, y, z;       /* owner voxel, global index */
    uint8_t r, g, b, label;
    uint8_t edge, pad[3];   /* class 1..7; pad = 0 */
} semtsdf_mesh_vertex;
int semtsdf_extract_mesh(semtsdf_vol* v, int32_t min_weight, semtsdf_mesh_vertex* verts, uint64_t vcap,
                         uint32_t* tris /* 3 per triangle */, uint64_t tcap /* triangles */,
                         uint64_t* nverts, uint64_t* ntris);

/* ---- instance inventory and id remapping (no reference counterpart) ----------------------------
 * semtsdf_instance_stats: what the semantic map contains, per instance id, in one read-only pass.
 * Selection: exactly that of semtsdf_export_surface -- every stored voxel this handle owns (a
 *   shard: its owned planes; never a halo plane, never the y/z padding of the tiled storage, never
 *   a plane with global z >= Dz) with weight >= min_weight and |sdf| < sdf_max (normalised units).
 * Label of a selected voxel: the argmax of its histogram, first maximum; 0 without a count.  So
 *   the sum of out[k].voxels over k equals semtsdf_export_surface's count for the same arguments.
 * out[k], 0 <= k < 32: see the fields below; sums run over the selected voxels labelled k, except
 *   `support`, which counts the selected voxels whose bin k is nonzero (labelled k or not).
 * overlap (optional, 32 x 32 u64, row-major): overlap[a * 32 + b] = the selected voxels in which
 *   bins a and b are both nonzero; symmetric, its diagonal is `support`.  NULL: not computed.
 * Everything is an integer, so the result does not depend on the order of accumulation: two calls
 *   on one state return identical bytes, and the shards' results add up (sums; min/max for the
 *   boxes) to the single volume's.  Outputs are host pointers; the call synchronises; the volume is
 *   not modified; scratch (11 KB) lives for the call.  A volume without SEMTSDF_F_SEMANTIC:
 *   SEMTSDF_ERR_UNSUPPORTED.  NULL v or out, or !(sdf_max > 0): SEMTSDF_ERR_INVALID, decided before
 *   any device work. */
typedef struct semtsdf_instance {   /* 96 bytes */
    uint64_t voxels;      /* selected voxels whose label is this id */
    uint64_t votes;       /* sum over those voxels of the winning bin's count */
    uint64_t support;     /* selected voxels whose bin of this id is nonzero (= overlap[id][id]) */
    uint64_t sum[3];      /* sums of the global voxel index (x, y, z) over `voxels` */
    uint64_t rgb_sum[3];  /* sums of the colour (int32 colours clamped to [0, 255]) over `voxels` */
    uint32_t min[3], max[3]; /* index bounding box of `voxels`; voxels == 0: min = UINT32_MAX, max = 0 */
} semtsdf_instance;
int semtsdf_instance_stats(semtsdf_vol* v, float sdf_max, int32_t min_weight,
                           semtsdf_instance out[SEMTSDF_MAX_OBJECTS], uint64_t* overlap /* [32*32] or NULL */);
/* semtsdf_remap_instances: the histogram through a lookup table, in place: merge, drop, compact ids.
 * For every stored voxel of the handle (halo planes included, so shards given the same table stay
 *   consistent with their neighbours): hist'[j] = sum of hist[k] over the k with lut[k] == j (u32,
 *   modulo 2^32); the bin mask the samplers use is rebuilt (bin j present iff hist'[j] != 0).  sdf,
 *   weight, colour, the steady flags, the empty-space maps and n_obs are untouched.
 * lut: lut[k] < 32 for every k and lut[0] == 0 (background stays background).  Any other id may map
 *   to 0 (dissolved into the background), to another id (merged) or to itself; cycles (a <-> b) are
 *   legal: every source bin of a voxel is read before any of its bins is written.
 * num_objs: -1 keeps the handle's next id; otherwise it becomes the next id (written in stream
 *   order) and, with cur the current one, must satisfy
 *     1 + max{lut[k] : 0 <= k < max(1, min(cur, 32))} <= num_objs <= max(cur, 1)
 *   (with -1 the left inequality is checked against max(cur, 1): no live id may map past the ids
 *   in use).  A violation of this or of the table rules: SEMTSDF_ERR_INVALID, nothing applied.
 * A volume without SEMTSDF_F_SEMANTIC: SEMTSDF_ERR_UNSUPPORTED.  The remap is queued on `stream`
 *   (NULL: the handle's own) as an integrate is: after the last empty-space map update and, in
 *   stream order, after the frame work queued before it (a frame's lagged view and deferred mask
 *   relabel are queued with that frame); readers on other streams are the caller's to order, as
 *   for semtsdf_parse_frame_dev_after.  The call itself reads the current next id, so it waits for
 *   the work queued before it on `stream`; it does not wait for the remap.  An identity table
 *   launches no kernel but still applies num_objs.
 * Merging is safe for the association: a voxel receives at most one vote per integrated frame, so
 *   the sum of any set of its bins is at most n_obs; a merged count therefore never exceeds what the
 *   reference could have produced, and the positive-term path of the association (a count above
 *   n_obs) is not triggered by a merge. */
int semtsdf_remap_instances(semtsdf_vol* v, const uint8_t lut[SEMTSDF_MAX_OBJECTS], int32_t num_objs,
                            void* stream);

/* ---- brick paging: occupied bricks out to the host and back (no reference counterpart) ----------
 * Bricks and voxels.  Brick b = (bx, by, bz), 0 <= b[a] < nb[a] = ceil(dim[a] / 8), holds the voxels
 *   8 b[a] <= i[a] < 8 b[a] + 8.  A voxel is real iff i[a] < dim[a] on every axis.  Voxel (x, y, z)
 *   has place w = 64 (x & 7) + 8 (y & 7) + (z & 7) in its brick.
 * Reset state, occupancy.  The reset state of a voxel is what semtsdf_reset leaves: sdf bits equal to
 *   those of mu; weight, colour, all 32 histogram bins, cls and cls_cnt 0.  A brick is occupied iff
 *   some real voxel of it differs from the reset state in any field the volume has (floats compared
 *   as bits).  bins of a brick is the OR over its real voxels of
 *   (hist[k] != 0) << k; 0 for a volume without SEMTSDF_F_SEMANTIC.
 * Record.  The record of a brick is made of u32 planes of 512 words, each in place order w:
 *   1. sdf bits;  2. weight as i32;
 *   3. colour: one plane r | g << 8 | b << 16 for u8 volumes, three planes r, g, b as i32 for
 *      SEMTSDF_F_COLOR_I32 volumes (whatever the current storage form is);
 *   4. one plane of hist[k] for every set bit k of bins, ascending;
 *   5. cls, then cls_cnt, for SEMTSDF_F_VOTE volumes.
 *   Voxels that are not real hold the reset state in the record.  A record does not depend on
 *   whether weights or colour are currently stored narrow or wide.
 * semtsdf_pack_bricks: the occupied bricks of the box lo <= b < hi (brick units) in ascending
 *   (bx, by, bz) order, z fastest; records back to back, offset (in words) the running sum.  A box
 *   outside 0 <= lo <= hi <= nb: SEMTSDF_ERR_INVALID; an empty box is legal.  Outputs are host
 *   pointers; the call synchronises.  bricks == NULL && words == NULL: count only (one NULL alone is
 *   SEMTSDF_ERR_INVALID).  With both given and a capacity short: SEMTSDF_ERR_INVALID, the counts
 *   written, the buffers untouched.  The volume and its derived state are not modified; the call
 *   orders itself after the work queued on the handle; two calls on one state return identical bytes.
 * semtsdf_unpack_bricks: overwrites the real voxels of the listed bricks with their records.  Planes
 *   of bins not in `bins` become 0, the bin mask is rebuilt per voxel from the written values;
 *   padding voxels and every other brick stay untouched.  Checked before any device work, each
 *   SEMTSDF_ERR_INVALID with nothing applied: a coordinate out of range; bricks not strictly
 *   ascending (so no duplicates); offsets that are not the running sum, or a total other than
 *   n_words; bins != 0 on a volume without SEMTSDF_F_SEMANTIC.  As semtsdf_upload: it runs after the
 *   last map update, the volume widens first if a weight does not fit u16 or an i32 colour lies
 *   outside [0, 255], the bound of the weights is raised (never lowered), the steady flags of every
 *   touched line are cleared, the empty-space maps are rebuilt before their next use, and the call
 *   synchronises.  n_bricks == 0 returns at once.
 * Both: a Z-sharded handle is SEMTSDF_ERR_UNSUPPORTED.  Staging (8 B, and to fill 24 B, per brick
 *   of the box; at most 256 MiB of records, or one record, at a time) comes from the handle's pool:
 *   it is counted in device_bytes while the call runs and released before it returns; failing to get
 *   it is SEMTSDF_ERR_OOM with the volume untouched. */
typedef struct semtsdf_brick { /* 24 bytes */
    int32_t b[3];
    uint32_t bins;
    uint64_t offset; /* of the record, in words */
} semtsdf_brick;
int semtsdf_pack_bricks(semtsdf_vol* v, const int32_t lo[3], const int32_t hi[3], semtsdf_brick* bricks,
                        uint64_t brick_capacity, uint32_t* words, uint64_t word_capacity, uint64_t* n_bricks,
                        uint64_t* n_words);
int semtsdf_unpack_bricks(semtsdf_vol* v, const semtsdf_brick* bricks, uint64_t n_bricks, const uint32_t* words,
                          uint64_t n_words);

/* ---- empty-space maps (tests) ------------------------------------------------------------
 * The octant distance map of the current volume state, one word per 8^3 brick (x-major, z
 * fastest): byte o = the octant-o distance in bricks (0: the brick is not skippable).  count =
 * the number of bricks (0: the handle has no octant maps); out may be NULL.  Synchronises. */
int semtsdf_map_words(semtsdf_vol* v, uint64_t* out, uint64_t capacity, uint64_t* count);

/* ---- measurement ------------------------------------------------------------------------ */
/* enable bit0: record HIP events around kernels; bit1: count touched/gated voxels; bit2: every
 * association row takes the exact f32 path (tests and its cost measurement); bits 3 and 4:
 * reserved, ignored (they selected experiment paths that have been removed). */
int semtsdf_set_instrumentation(semtsdf_vol* v, int enable);
int semtsdf_get_timing(semtsdf_vol* v, semtsdf_timing* out); /* synchronises the stream */
int semtsdf_reset_timing(semtsdf_vol* v);

/* ---- drop-in for tsdf_cuda.tsdf_update (TSDF_Python/tsdf.cpp:11-33, exact argument order) --
 * Host arrays updated in place: tsdf_diff f32[D^3], tsdf_color i32[D^3*3], tsdf_wt i32[D^3],
 * tsdf_cls i32[D^3], tsdf_cls_cnt i32[D^3]; vol_start f32[3]; intrinsic f32[16];
 * depth u16[H*W]; color u8[H*W*3]; cls i32[H*W]; extrinsic2init f32[16]. */
int semtsdf_tsdf_update(float* tsdf_diff, int32_t* tsdf_color, int32_t* tsdf_wt, int32_t* tsdf_cls,
                        int32_t* tsdf_cls_cnt, int vol_dim, const float* vol_start, float voxel,
                        float miu, const float* intrinsic, const uint16_t* depth, const uint8_t* color,
                        const int32_t* cls, const float* extrinsic2init, int width, int height);

#ifdef __cplusplus
}
#endif
#endif /* SEMTSDF_H */
