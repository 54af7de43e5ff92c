/* include/pwpp.h -- C-ABI of the MI355X-native Patchwork++ hot path (libpwpp_hip.so).
 *
 * This is the drop-in boundary for the reference's per-frame path
 *     patchwork::PatchWorkpp::estimateGround()      /root/reference/cpp/patchworkpp/src/patchworkpp.cpp:151-336
 * and its result getters                            /root/reference/cpp/patchworkpp/include/patchwork/patchworkpp.h:152-163
 * Plain C: POD structs, raw pointers and sizes only; no C++ / torch / Eigen types cross it.
 * The reference has no FFI of its own for this path (its Python module binds the C++ class
 * directly, python/patchworkpp/pybinding.cpp:45-55); the C++ class and pybind11 module that
 * sit on top of this header (patchwork-plusplus_amd/include/patchwork/patchworkpp.h,
 * patchwork-plusplus_amd/python/pybinding.cpp) are what a maintainer would swap in --
 * see INTEGRATION.md.
 *
 * Every entry point returns PWPP_OK (0) or a negative pwpp_status; pwpp_last_error() gives
 * the text for the calling thread.  One handle = one device + one HIP stream; a handle is
 * not re-entrant (like the reference object, patchworkpp.h:177-195), distinct handles are
 * independent and may be driven from different threads.
 */
#ifndef PWPP_H
#define PWPP_H

#include <stdint.h>

/* Only the entry points below are exported: libpwpp_hip.so is built with -fvisibility=hidden. */
#ifndef PWPP_API
#define PWPP_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define PWPP_VERSION_MAJOR 0
#define PWPP_VERSION_MINOR 4 /* per-point patch rows and plane distances (pwpp_set_point_planes, pwpp_get_*point_*) */

typedef enum pwpp_status {
    PWPP_OK = 0,
    PWPP_E_ARG = -1,         /* bad argument / parameter combination              */
    PWPP_E_HIP = -2,         /* a HIP runtime call failed                          */
    PWPP_E_NOMEM = -3,       /* device or host allocation failed                   */
    PWPP_E_STATE = -4,       /* call sequence error (e.g. getter before any frame) */
    PWPP_E_UNSUPPORTED = -5, /* legal for the reference, not implemented here      */
    PWPP_E_NODEVICE = -6     /* no usable GPU: the product path never falls back to CPU */
} pwpp_status;

/* Mirror of patchwork::Params, field for field (reference patchworkpp.h:42-112).
 * bools are int32 (0/1); the four std::vector members are fixed arrays of 4 because the
 * reference hard-codes four zones (patchworkpp.h:122-134, patchworkpp.cpp:580-615). */
typedef struct pwpp_params {
    int32_t verbose;      /* patchworkpp.h:44 */
    int32_t enable_RNR;   /* :45 */
    int32_t enable_RVPF;  /* :46 */
    int32_t enable_TGR;   /* :47 */
    int32_t num_iter;     /* :49 */
    int32_t num_lpr;      /* :50 */
    int32_t num_min_pts;  /* :51 */
    int32_t num_zones;    /* :52  (must be 4, see above) */
    int32_t num_rings_of_interest; /* :53 (<= 4: the reference keeps update_*_[4], patchworkpp.h:174-175) */
    int32_t pad0_;
    double RNR_ver_angle_thr; /* :55 */
    double RNR_intensity_thr; /* :56 */
    double sensor_height;     /* :58 */
    double th_seeds;          /* :59 */
    double th_dist;           /* :60 */
    double th_seeds_v;        /* :61 */
    double th_dist_v;         /* :62 */
    double max_range;         /* :63 */
    double min_range;         /* :64 */
    double uprightness_thr;   /* :65 */
    double adaptive_seed_selection_margin; /* :66 */
    double intensity_thr;     /* :67 (never read by the hot path; kept for API parity) */
    int32_t num_sectors_each_zone[4]; /* :69 */
    int32_t num_rings_each_zone[4];   /* :70 */
    int32_t max_flatness_storage;     /* :72 */
    int32_t max_elevation_storage;    /* :73 */
    double elevation_thr[4];          /* :75 */
    double flatness_thr[4];           /* :76 */
} pwpp_params;

/* Adaptive per-stream state the reference keeps inside the object and mutates every frame
 * (params_.sensor_height / elevation_thr / flatness_thr, patchworkpp.cpp:347-350,368). */
typedef struct pwpp_state {
    double sensor_height;
    double elevation_thr[4];
    double flatness_thr[4];
    int32_t elevation_len[4]; /* entries in update_elevation_[i] */
    int32_t flatness_len[4];  /* entries in update_flatness_[i]  */
} pwpp_state;

/* One processed patch (CZM bin with >= num_min_pts points), in bin traversal order. */
typedef struct pwpp_patch_record {
    int32_t bin;            /* flattened zone->ring->sector index (patchworkpp.cpp:184-189) */
    int32_t concentric_idx; /* patchworkpp.cpp:174,309 */
    int32_t n_points;
    int32_t n_ground;       /* |regionwise_ground_|     (patchworkpp.cpp:529-531) */
    int32_t n_nonground;    /* |regionwise_nonground_|  (patchworkpp.cpp:500,532) */
    int32_t decision;       /* pwpp_decision */
    float mean[3];          /* pc_mean_            (patchworkpp.cpp:59-60) */
    float normal[3];        /* normal_             (patchworkpp.cpp:66-68) */
    float sv[3];            /* singular_values_    (patchworkpp.cpp:63)    */
    int32_t rounds;         /* diagnostic, no reference counterpart: R-GPF rounds the fit ran -- num_iter, or fewer when a round's
                             * integer totals repeated the round before's (early termination: the remaining rounds and the final fit
                             * of patchworkpp.cpp:516-543 provably reproduce this round's set and plane) */
    double d;               /* d_                  (patchworkpp.cpp:74)    */
} pwpp_patch_record;

typedef enum pwpp_decision {
    PWPP_DEC_NOT_UPRIGHT = 1, /* patchworkpp.cpp:262-265 */
    PWPP_DEC_FAR_GROUND = 2,  /* :266-269 */
    PWPP_DEC_HEADING = 3,     /* :270-273 */
    PWPP_DEC_GROUND = 4,      /* :274-277 */
    PWPP_DEC_TGR_REJECT = 5,  /* :278-282 then :452-459 / :296-300 */
    PWPP_DEC_TGR_REVERT = 6   /* :444-451 */
} pwpp_decision;

enum { PWPP_LAYOUT_ROW_MAJOR = 0, /* (n, cols) C-order: np.fromfile(..).reshape(-1,4), python/examples/demo_visualize.py:10-14 */
       PWPP_LAYOUT_COL_MAJOR = 1, /* Eigen::MatrixXf default storage: cols planes of n floats (patchworkpp.h:152) */
       PWPP_LAYOUT_FIELDS = 2     /* (internal to pwpp_estimate_ground_fields*: float32 fields at byte offsets of a record) */ };
enum { PWPP_MEM_HOST = 0,         /* pageable or pinned host memory; the call returns when the results are ready */
       PWPP_MEM_DEVICE = 1,       /* device memory; asynchronous */
       PWPP_MEM_HOST_PINNED = 2   /* page-locked host memory (pwpp_host_alloc / hipHostMalloc) that stays valid and
                                     unchanged until pwpp_synchronize(): the copies and the launches are only
                                     enqueued, so a second handle can overlap its own transfers and kernels
                                     (double-buffered ingest) */ };
enum { PWPP_MODE_FRESH = 0,   /* every frame starts from the handle's Params (= a fresh PatchWorkpp object per frame) */
       PWPP_MODE_STREAMS = 1  /* frame i belongs to stream i and reads+updates that stream's adaptive state
                                 (= one long-lived PatchWorkpp object per stream, demo_sequential.cpp:54-67) */ };

typedef struct pwpp_handle pwpp_handle;

/* ---- lifetime ------------------------------------------------------------------------- */
/* Params() defaults, reference patchworkpp.h:79-111 */
PWPP_API int pwpp_params_default(pwpp_params *p);
/* PatchWorkpp::PatchWorkpp(Params), reference patchworkpp.h:120-150: validates, computes the
 * CZM geometry in double exactly as the reference constructor, creates stream + workspace. */
PWPP_API int pwpp_create(const pwpp_params *p, int device, pwpp_handle **out);
PWPP_API int pwpp_destroy(pwpp_handle *h);
PWPP_API const char *pwpp_last_error(void);
PWPP_API int pwpp_device_count(void);

/* ---- the hot path ---------------------------------------------------------------------- */
/* void PatchWorkpp::estimateGround(Eigen::MatrixXf cloud_in), reference patchworkpp.cpp:151.
 * One frame, host memory, stream 0 of the handle, stateful like the reference object.
 * cols is 3 or 4 (3 only legal with enable_RNR == 0 semantics of patchworkpp.cpp:379-382:
 * RNR is skipped).  Synchronous: results are ready on return. */
PWPP_API int pwpp_estimate_ground(pwpp_handle *h, const float *points, int n, int cols, int layout);

/* Many independent frames in one set of launches.  points[i] is frame i (host or device
 * memory according to `mem`), n[i] its point count.  PWPP_MODE_FRESH: each frame is
 * processed with fresh state.  PWPP_MODE_STREAMS: frames <= streams configured with
 * pwpp_set_num_streams(); frame i continues stream i.  Asynchronous when mem is
 * PWPP_MEM_DEVICE or PWPP_MEM_HOST_PINNED: call pwpp_synchronize() before reading results. */
PWPP_API int pwpp_estimate_ground_batch(pwpp_handle *h, const float *const *points, const int32_t *n, int frames,
                               int cols, int layout, int mem, int mode);
/* The ROS 2 wrapper's input (reference ros/src/GroundSegmentationServer.cpp:72-75, ros/src/Utils.hpp:158-172
 * PointCloud2ToEigenMat: x, y, z read through one float32 iterator per field): `data` = msg->data, n = height * width,
 * point_step and the byte offsets of the fields as the message declares them (4-byte aligned; off_intensity < 0 when
 * there is none -- RNR is then skipped as for an N x 3 matrix, patchworkpp.cpp:379-382).  The fields are read where
 * they lie: no repacked copy on the host.  pwpp_estimate_ground_fields = one frame on stream 0 from host memory, like
 * pwpp_estimate_ground; the _batch form takes `mem` and `mode` like pwpp_estimate_ground_batch. */
PWPP_API int pwpp_estimate_ground_fields(pwpp_handle *h, const void *data, int n, int point_step, int off_x, int off_y, int off_z, int off_intensity);
PWPP_API int pwpp_estimate_ground_fields_batch(pwpp_handle *h, const void *const *data, const int32_t *n, int frames, int point_step,
                                      int off_x, int off_y, int off_z, int off_intensity, int mem, int mode);
PWPP_API int pwpp_synchronize(pwpp_handle *h);
PWPP_API int pwpp_set_num_streams(pwpp_handle *h, int streams); /* (re)creates `streams` fresh stream states */

/* ---- results of the last call ---------------------------------------------------------- */
/* sizes of getGround()/getNonground()/getCenters(), reference patchworkpp.h:157-163 */
PWPP_API int pwpp_get_counts(pwpp_handle *h, int frame, int32_t *n_ground, int32_t *n_nonground, int32_t *n_patches);
/* getGroundIndices()/getNongroundIndices(), reference patchworkpp.h:159-160, patchworkpp.cpp:18-26.
 * The index SETS are those of the reference's control flow with the plane-fit sums of patchworkpp.cpp:56-60
 * evaluated (contract v4)
 *   - for a fit set of 1, 2 or 3 points: in the reference's own float arithmetic, which is determinate there (Eigen
 *     reduces fewer elements than one SIMD packet sequentially; two terms commute) -- points in the order of the
 *     reference's z-sorted bin, equal heights in cloud order (the reference's std::sort is stable only for bins of up
 *     to 16 points -- libstdc++'s insertion sort; beyond that members of EQUAL height may reach it in another order, and
 *     the last bits of a 2-3 point float mean / covariance with them: the bit-for-bit statement holds for distinct heights,
 *     tests/test_tiny_fits.py records the behaviour with duplicated heights).  All three builds of the reference under oracle/_ref agree
 *     on such sets and this library agrees with them: identical ground sets under the ROS launch file's parameters,
 *     num_min_pts 0-3, num_lpr 1-3 on the KITTI samples (tests/test_tiny_fits.py, CPU and GPU);
 *   - for 4 points and more: in EXACT arithmetic on the reference's own floats -- integer moments on a 2^-30 m grid around
 *     per-bin / per-patch origins, on which every float of magnitude >= 2^-7 m lies (smaller ones are rounded to it: an error of
 *     at most 2^-31 m); z clamped to z0 +- 2^(35-s) m = 32 m with the default CZM (pwpp_get_fxp_geometry).  Eigen's float
 *     summation order there depends on the vector width it was built for; exact sums do not depend on any order, and they are what
 *     every order approximates.  Bit-identical to the CPU restatement of the contract (oracle/).
 *     Measured on 10 400 frames against all three builds of the reference (float sums in two orders, exact-f64 sums; tools/parity_statistics.py,
 *     profiles/r06_parity_statistics_10k.json -- CPU restatement of the contract, which the HIP path equals bit for bit): 6 000 varied 64-beam
 *     frames with fresh state, 20 stateful sequences of 200 frames, 400 dense 128-beam frames with the 36-sector CZM.  The builds are
 *     unanimous on 5 829 / 3 869 / 334 of them, and this library returns exactly their ground set on EVERY one of those 10 032 frames.
 *     Where the builds differ among themselves (2.9 % / 3.3 % / 16.5 % of the frames: there is no single reference result) the library
 *     equals one of the builds on all 368: the exact-f64 build on 303, both float builds on 63 (frames where a fit set of 1-3 points
 *     decides -- the reference sums those in float, determinately; the exact-f64 build is the odd one out there), one float build on 2.
 *     Adaptive sensor height over the 200-frame sequences: within 1.2e-3 m of the exact build, as the float build of the reference is
 *     (a split frame's differing patch decision enters the elevation history).  On the reference's own KITTI samples: identical index
 *     sets with every build, plane normals within 3.1e-5 of the float build's and 6e-8 of the exact build's.
 *     Option "exact_moments" = 0 selects rounds 3-5's coarser 2^-21 m grid (contract v3: |Q| <= 2^26, nine multiply-adds per point instead of
 *     twenty-one): 7 % faster on 1024-frame batches (2.36 vs 2.52 ms per batch on one MI355X), 5-6 us on a single frame -- and off the unanimous
 *     reference by 1-31 indices of ~120 000 on 0.2 % of varied frames (18 of the 10 032 above), because that grid is coarser than the float
 *     ulp of heights around -1.7 m and of |x|, |y| < 4 m.  Both widths are tested bit for bit against their restatements.
 * (NaN heights are undefined in the reference itself: it sorts bins with `a.z < b.z`.)
 * The order inside a list is not the reference's unless pwpp_set_output_order asks for it. */
PWPP_API int pwpp_get_ground_indices(pwpp_handle *h, int frame, int32_t *out);
PWPP_API int pwpp_get_nonground_indices(pwpp_handle *h, int frame, int32_t *out);
/* getGround()/getNonground(), reference patchworkpp.h:157-158: row-major (count,3) float32,
 * rows aligned with the index getters above.  The rows are gathered from the frame's input when these getters are
 * called: after a PWPP_MEM_DEVICE call that input is the caller's device buffer, which must therefore still hold the
 * frame (unchanged, not freed) when they run.  The index getters have no such need.  With input transforms set
 * (pwpp_set_input_transforms) the rows are the TRANSFORMED coordinates, those the call ran on. */
PWPP_API int pwpp_get_ground_xyz(pwpp_handle *h, int frame, float *out);
PWPP_API int pwpp_get_nonground_xyz(pwpp_handle *h, int frame, float *out);
/* getCenters()/getNormals(), reference patchworkpp.h:162-163: row-major (n_patches,3), bin traversal order */
PWPP_API int pwpp_get_centers(pwpp_handle *h, int frame, float *out);
PWPP_API int pwpp_get_normals(pwpp_handle *h, int frame, float *out);
/* per-patch detail for parity checks (no reference getter; fields are the reference's scratch members) */
PWPP_API int pwpp_get_patch_records(pwpp_handle *h, int frame, pwpp_patch_record *out, int capacity);
/* getHeight(), reference patchworkpp.h:154 (stream 0) */
PWPP_API double pwpp_get_height(pwpp_handle *h);
/* getTimeTaken(), reference patchworkpp.h:155: microseconds of the last estimate call
 * (GPU time between HIP events on the handle's stream, batch calls: whole batch: first kernel -> index lists written.  With up to 64
 * stateful streams the update of the streams' adaptive thresholds -- K5's second launch, option "split_k5" -- runs on the handle's second
 * stream and ends ~8 us after the lists; the next estimate call and every call that touches a stream's state wait for it, pwpp_synchronize
 * and the getters of a call's results -- counts, lists, patch rows -- do not) */
PWPP_API double pwpp_get_time_us(pwpp_handle *h);

/* ---- adaptive state --------------------------------------------------------------------- */
/* state after the last call; PWPP_MODE_FRESH: `index` is the frame, PWPP_MODE_STREAMS: the stream */
PWPP_API int pwpp_get_state(pwpp_handle *h, int index, pwpp_state *out);
PWPP_API int pwpp_get_history(pwpp_handle *h, int index, int which /*0 elevation, 1 flatness*/, int ring, double *out, int capacity);
/* overwrite the scalars of a stream state; its histories are cleared (elevation_len / flatness_len of `in` are ignored),
 * its plane members (pwpp_set_plane_state) are left as they are */
PWPP_API int pwpp_set_state(pwpp_handle *h, int stream, const pwpp_state *in);
/* ... and put a history back: after pwpp_set_state + eight pwpp_set_history calls with what pwpp_get_state /
 * pwpp_get_history returned, a stream continues exactly where the checkpointed one stood. */
PWPP_API int pwpp_set_history(pwpp_handle *h, int stream, int which /*0 elevation, 1 flatness*/, int ring, const double *values, int count);
/* The plane members of the reference object (pc_mean_, normal_, singular_values_, d_: patchworkpp.h:177-182) as they
 * stand after the state's last frame -- {mean[3], normal[3], singular values[3], d}.  They are part of what a stream
 * carries from frame to frame: a bin that is processed without a fit (an empty bin let through by num_min_pts <= 0, the
 * ROS launch file's setting) reports whatever plane was fitted last, also across frames (patchworkpp.cpp:49).  Zero for a
 * new stream; a checkpoint is pwpp_get_state + the histories + this. */
PWPP_API int pwpp_get_plane_state(pwpp_handle *h, int index, float out[10]);
/* Frames this handle had to finish with the serial fix-up kernel: a patch whose first fit set is empty consults the
 * plane the reference object fitted last (the patch before it, or the frame before), which the parallel fit kernels
 * only recognise; the host then runs k_fit_fixup + the GLE and list kernels for that frame.  It takes a lowest height
 * of -inf, one beyond 1e15 m, or num_lpr = 0 -- no real scan; the count exists for tests. */
PWPP_API int64_t pwpp_get_fixed_up_frames(pwpp_handle *h);
/* Frames this handle has seen in which the FINAL ground set of some patch held a height outside z0 +- 2^(26-s) m (32 m with
 * the default CZM), i.e. a fit of 4+ points whose z coordinates were clamped before they were quantised (see
 * pwpp_get_fxp_origins): that patch's plane is the plane of the clamped heights, not the reference's.  No ground patch is
 * that tall; a steep facade or cliff filling a bin can be (it is rejected as "not upright" either way with the default
 * parameters).  0 on every scan of the test suite.  (2^(35-s) with the default "exact_moments" = 1, 2^(26-s) with 0: 32 m either way
 * for the default CZM, s = 30 / 21.) */
PWPP_API int64_t pwpp_get_clamped_frames(pwpp_handle *h);
/* Host only (no device needed): shift and per-bin origins {ox, oy} of the fixed-point plane-fit sums a handle created with
 * these parameters uses by default (= pwpp_get_fxp_shift / pwpp_get_fxp_origins of that handle; contract v4: s <= 30, |Q| <= 2^35.
 * The origins do not depend on the option "exact_moments"; the shift does -- pwpp_get_fxp_shift reports the handle's current one).  The CPU tests compare them with
 * the restatement's for many CZM shapes.  Returns the number of bins; shift / out_xy may be NULL. */
PWPP_API int pwpp_get_fxp_geometry(const pwpp_params *p, int *shift, float *out_xy, int capacity_bins);
/* Host only (no device needed): the axis-aligned box {xmin, xmax, ymin, ymax} the library assumes around every CZM bin of
 * a parameter set, bins in traversal order (zone, ring, sector).  The fit kernels prove with it that no point of a bin's
 * high part can lie below a plane, so every point the reference bins into b must lie inside box b:
 * tests/test_capi_cpu.py checks exactly that.  Returns the number of bins (with out_boxes == NULL: just that). */
PWPP_API int pwpp_get_bin_boxes(const pwpp_params *p, float *out_boxes, int capacity_bins);
PWPP_API int pwpp_set_plane_state(pwpp_handle *h, int stream, const float in[10]);

/* ---- ingest ----------------------------------------------------------------- */
/* Page-locked host memory: frames handed over in such buffers are DMA'd straight to the device
 * (pageable memory is staged by the runtime at a fraction of the PCIe rate), and result copies
 * into them do not block. */
PWPP_API int pwpp_host_alloc(void **out, uint64_t bytes);
PWPP_API int pwpp_host_free(void *p);
/* All index lists of the last batch in ONE device-to-host copy: out[frame_base[f] .. +n_ground)
 * is frame f's ground list, followed by its non-ground list; frame_base (frames+1 entries) and
 * counts (frames x 8 int32, see pwpp_device_view) are filled if not NULL.  `out` must hold the
 * total number of points of the batch. */
PWPP_API int pwpp_get_all_indices(pwpp_handle *h, int32_t *out, int64_t *frame_base, int32_t *counts);

/* ---- device-side views and measurement --------------------------------------------------- */
typedef struct pwpp_device_view {
    const int32_t *indices;      /* all frames: [frame_base[f] .. +n_ground) ground, then nonground */
    const int64_t *frame_base;   /* frames+1 prefix sums of n (host pointer, pinned)                */
    const int32_t *counts;       /* frames x 8 int32 (host pointer, pinned): n_ground, n_nonground, n_patches, n_rnr, n_out_of_range, n_dropped,
                                    history fill (library bookkeeping), 0 */
    int32_t frames;
    int32_t pad_;
} pwpp_device_view;
PWPP_API int pwpp_get_device_view(pwpp_handle *h, pwpp_device_view *out);

/* per-kernel GPU time (HIP events on the handle's stream around every launch) */
#define PWPP_NUM_KERNELS 11
PWPP_API int pwpp_set_profiling(pwpp_handle *h, int enable);
PWPP_API int pwpp_get_kernel_profile(pwpp_handle *h, double *sum_ms /*[PWPP_NUM_KERNELS]*/, int64_t *launches /*[PWPP_NUM_KERNELS]*/);
PWPP_API int pwpp_reset_kernel_profile(pwpp_handle *h);
PWPP_API const char *pwpp_kernel_name(int k);
/* the fixed-point contract of the plane-fit sums for this handle: the shift s (grid 2^-s m) ... */
PWPP_API int pwpp_get_fxp_shift(pwpp_handle *h);
/* ... and every bin's origin (its polar centre rounded to 1/8 m): out_xy = B x {x, y}; returns B (out_xy = NULL: only B).
 * The z coordinates of a fit of 4+ points are clamped to z0 +- 2^(35-s) m (32 m with the default CZM; z0 = the patch's first
 * lowest-point representative rounded to 1/8 m) before they are quantised: a fit set that spans more than that vertically --
 * no ground patch does; a facade that R-VPF did not strip could -- gets the plane of the clamped heights. */
PWPP_API int pwpp_get_fxp_origins(pwpp_handle *h, float *out_xy, int capacity_bins);
/* Order of the points INSIDE a patch's part of the index lists (the parts themselves always follow the
 * reference: bin traversal order, TGR candidates at the end of their ring).
 *   PWPP_ORDER_SCATTER   (default) whatever the binning atomics produced -- same sets, fastest;
 *   PWPP_ORDER_REFERENCE the reference's order (patchworkpp.cpp:199 sorts a bin by z; :500,:532): ground
 *                        candidates ascending in z; non-ground: the points each R-VPF round removed, then
 *                        the rest, each ascending in z; small bins / RNR / out-of-range in cloud order.
 *                        Equal z (-0.0 and +0.0 are equal): cloud order (the reference's std::sort leaves ties unspecified).
 * Applies to the batches launched after the call. */
enum { PWPP_ORDER_SCATTER = 0, PWPP_ORDER_REFERENCE = 1, PWPP_ORDER_CLOUD = 2 };
PWPP_API int pwpp_set_output_order(pwpp_handle *h, int order);
/*   PWPP_ORDER_CLOUD     both lists in ascending cloud index (no per-patch layout): a function of the input alone.
 *                        Implies labels (below).  Every list getter, pwpp_get_all_indices and the device view follow it. */

/* ---- per-point labels (batches launched after pwpp_set_labels(h, 1) or with PWPP_ORDER_CLOUD) --------------------------
 * One byte per point, cloud order, laid out like the index lists (frame f at frame_base[f]).  UNCLASSIFIED = in neither
 * list: the reference's skip marker z == FLT_MIN (n_dropped).  RNR and out-of-range points are NONGROUND.  Computed on the
 * device behind the lists; their time counts in the k_emit slot of the kernel profile.  The getters return PWPP_E_STATE
 * when the last call ran without labels.  A pipe's handles take this and the order through pwpp_pipe_handle. */
enum { PWPP_LABEL_NONGROUND = 0, PWPP_LABEL_GROUND = 1, PWPP_LABEL_UNCLASSIFIED = 2 };
PWPP_API int pwpp_set_labels(pwpp_handle *h, int on);
PWPP_API int pwpp_get_labels(pwpp_handle *h, int frame, uint8_t *out);          /* n bytes of frame `frame` */
PWPP_API int pwpp_get_all_labels(pwpp_handle *h, uint8_t *out);                 /* the whole batch in ONE copy */
PWPP_API int pwpp_get_device_labels(pwpp_handle *h, const uint8_t **out);      /* device pointer; frame_base as in the device view */

/* ---- per-point patch rows and plane distances (batches launched after pwpp_set_point_planes(h, 1)) ---------------------
 * Two arrays, cloud order, laid out like the labels (frame f at frame_base[f]); independent of labels and of the output order.
 *   patch     int32: the row p of the point's patch in pwpp_get_patch_records / pwpp_get_centers / pwpp_get_normals, or -1.  A
 *             point belongs to patch p if the reference's pc2czm puts it into the bin of record p: its ground points, its
 *             regionwise non-ground points, the points R-VPF stripped and its TGR candidates (reverted or not).  -1: points of
 *             bins with fewer than num_min_pts points, RNR points, points outside (min_range, max_range], and the skip marker
 *             z == FLT_MIN (PWPP_LABEL_UNCLASSIFIED).  With num_min_pts <= 0 empty bins are patches (rows) that own no points.
 *   distance  float: the signed distance of the point to its patch's REPORTED plane -- the record's normal and d, i.e. the
 *             final estimate_plane of the patch (patchworkpp.cpp:541), which is what pwpp_get_normals shows -- or NaN where
 *             patch is -1.  The reference's calc_point_to_plane_d (:551-554) in its own operation order, rounded once:
 *                 s = fl32(fl32(fl32(n0 * x) + fl32(n1 * y)) + fl32(n2 * z));   dist = (float)((double)s + d)
 *             with x, y, z the input floats.  The normal has n2 >= 0, so a positive distance is above the plane.  This is
 *             not necessarily the plane of the last R-GPF round that made the ground / non-ground test; in a patch decided
 *             NOT_UPRIGHT it is a distance to a wall, not a height.  A patch with an inherited plane (num_min_pts <= 0, or a
 *             first fit set that was empty) gets that plane, as its record does; a patch whose ground set was clamped
 *             (pwpp_get_clamped_frames) gets the plane of the clamped heights.  A NaN or inf coordinate gives what IEEE
 *             arithmetic gives.
 * Computed on the device behind the lists; their time counts in the k_emit slot of the kernel profile.  The getters return
 * PWPP_E_STATE when the last call ran without point planes.  A pipe's handles take the setting through pwpp_pipe_handle. */
PWPP_API int pwpp_set_point_planes(pwpp_handle *h, int on);
PWPP_API int pwpp_get_point_patches(pwpp_handle *h, int frame, int32_t *out);       /* n entries of frame `frame` */
PWPP_API int pwpp_get_point_distances(pwpp_handle *h, int frame, float *out);       /* n entries of frame `frame` */
PWPP_API int pwpp_get_all_point_patches(pwpp_handle *h, int32_t *out);              /* the whole batch in ONE copy */
PWPP_API int pwpp_get_all_point_distances(pwpp_handle *h, float *out);              /* the whole batch in ONE copy */
/* device pointers (either may be NULL); frame_base as in the device view */
PWPP_API int pwpp_get_device_point_planes(pwpp_handle *h, const int32_t **patches, const float **distances);

/* ---- whole records of the ground / non-ground points (pwpp_set_point_records, pwpp_get_*_records) ------------------------
 * getGround() / getNonground() (reference patchworkpp.h:157-158) with everything the input carried: row r of a list is the
 * record of the point the index getter names at r, in whatever output order the handle has.  The row size is the same for
 * every frame of a call, pwpp_get_record_bytes():
 *   PWPP_LAYOUT_ROW_MAJOR   cols * 4       the input row
 *   PWPP_LAYOUT_COL_MAJOR   cols * 4       {x, y, z[, w]} gathered from the planes, row-major
 *   pwpp_estimate_ground_fields*  point_step   the point verbatim: every byte, padding and the fields the library never reads included
 * Bytes are copied, never interpreted: NaN payloads, -0.0 and integer fields (ring, time stamps) arrive as they were.
 * pwpp_get_ground_records / pwpp_get_nonground_records fill count x record_bytes bytes and work after every call:
 *   - after a call launched with pwpp_set_point_records(h, 1) the rows were written on the device behind the lists (their time
 *     counts in the k_emit slot of the kernel profile) and are only copied: the input is not touched again, so after a
 *     PWPP_MEM_DEVICE call the caller's buffer may be overwritten or freed;
 *   - otherwise they are gathered from the frame's input when the getter runs, as pwpp_get_ground_xyz does, under its lifetime
 *     rule: after a PWPP_MEM_DEVICE call the caller's buffer must still hold the frame.
 * pwpp_get_all_records (the whole batch in ONE copy) and pwpp_get_device_records (device pointer, nothing copied) need a last
 * call that ran with the setting on and return PWPP_E_STATE otherwise.  The buffer is laid out like the index lists, in rows:
 * frame f starts at row frame_base[f] (byte frame_base[f] * record_bytes: 4-byte aligned, 16-byte aligned when record_bytes is a
 * multiple of 16), holds its n_ground ground rows, then its n_nonground non-ground rows; the frame's remaining n_dropped rows are
 * unspecified.  frame_base (frames + 1 entries) and counts (frames x 8 int32) as in pwpp_get_all_indices; either may be NULL.
 * `out` must hold total points x record_bytes bytes.  The device buffer stays valid until the handle's next estimate call,
 * pwpp_trim_workspace or pwpp_destroy.  The setting applies to the batches launched after the call; with it off nothing is
 * allocated or launched for it.  A pipe's handles take it through pwpp_pipe_handle. */
#define PWPP_HAS_POINT_RECORDS 1
PWPP_API int pwpp_set_point_records(pwpp_handle *h, int on);
PWPP_API int pwpp_get_record_bytes(pwpp_handle *h);   /* bytes per row of the last call; PWPP_E_STATE before any call */
PWPP_API int pwpp_get_ground_records(pwpp_handle *h, int frame, void *out);
PWPP_API int pwpp_get_nonground_records(pwpp_handle *h, int frame, void *out);
PWPP_API int pwpp_get_all_records(pwpp_handle *h, void *out, int64_t *frame_base, int32_t *counts);
PWPP_API int pwpp_get_device_records(pwpp_handle *h, const void **out, int32_t *record_bytes);   /* either may be NULL */

/* ---- the fitted ground model at arbitrary positions and as a grid (pwpp_query_ground, pwpp_rasterize_ground) ---------------
 * What pwpp_set_point_planes gives for the cloud's own points, for ANY position: the ground height under a detection box, the
 * height above ground of a return that was not part of the fit (radar, a second LiDAR), a bird's-eye elevation image.
 *   When      Both calls answer from the results of the handle's LAST estimate call and work after every kind of call (fresh or
 *             streams, any layout, memory kind and schedule, a pipe's handles); no setter is needed.  They enter like the getters:
 *             the call in flight lands first, a frame that awaits the serial fix-up or a redo is finished first.  PWPP_E_STATE
 *             before any call and after pwpp_trim_workspace.  Pure reads: no result, state or timing of the estimate path changes.
 *   mem       PWPP_MEM_HOST: input and output are host memory, staged through buffers of the handle; synchronous.
 *             PWPP_MEM_DEVICE: input and output are device memory, the work is enqueued on the handle's stream and is complete
 *             after pwpp_synchronize.  PWPP_MEM_HOST_PINNED: PWPP_E_ARG.
 *   bin       The bin the reference's pc2czm (patchworkpp.cpp:593-615) puts a point with these x, y into, all in double.  The
 *             query's z plays no part in it.  RNR and the skip marker z == FLT_MIN are tests on the points of a cloud and do NOT
 *             apply to positions -- consequence: a cloud point that RNR removed has patch -1 in pwpp_get_point_patches, but its
 *             position queries into its bin's patch.  The no-patch sample {-1, 0, NaN, NaN} answers: a position outside
 *             (min_range, max_range] or with a NaN / inf x or y; a position in a bin with fewer than num_min_pts points; an entry
 *             whose frame[i] is outside [0, frames of the last call) -- the kernel checks that, the host does not scan the list,
 *             so both memory kinds behave the same.
 *   patch     The row of the bin's patch in pwpp_get_patch_records / pwpp_get_centers / pwpp_get_normals: patch bins ranked in
 *             ascending bin order.  With num_min_pts <= 0 empty bins are rows too and answer with their inherited plane, as their
 *             record does.
 *   distance  The point-planes formula, unchanged, against the record's normal and d (the patch's REPORTED plane):
 *                 s = fl32(fl32(fl32(n0 * x) + fl32(n1 * y)) + fl32(n2 * z));   distance = (float)((double)s + d)
 *             A NaN or inf z gives what IEEE arithmetic gives.
 *   ground_z  The height of that plane at (x, y), in double on the record's floats, rounded once:
 *                 ground_z = (float)( -(((double)n0 * (double)x + (double)n1 * (double)y) + d) / (double)n2 )
 *             (the products are exact in double; one rounding per add, one IEEE division, one rounding to float).  n2 == 0 gives
 *             what IEEE gives; in a patch decided NOT_UPRIGHT it is the height of a wall's plane, not of ground: see `decision`.
 *   edge      m == 0 is PWPP_OK and launches nothing; a null xyz or out with m > 0 is PWPP_E_ARG.  Caller pointers need the natural
 *             alignment of their element types (4 bytes) and no more.
 * Nothing is allocated for this until the first query; pwpp_trim_workspace frees it and pwpp_get_workspace_bytes counts it. */
#define PWPP_HAS_GROUND_QUERY 1
typedef struct pwpp_ground_sample {   /* 16 bytes */
    int32_t patch;      /* row in pwpp_get_patch_records / centers / normals of the patch whose bin holds (x, y); -1: none */
    int32_t decision;   /* that record's pwpp_decision; 0 where patch is -1 */
    float   ground_z;   /* height of the patch's REPORTED plane at (x, y); NaN where patch is -1 */
    float   distance;   /* signed distance of (x, y, z) to that plane; NaN where patch is -1 */
} pwpp_ground_sample;
PWPP_API int pwpp_query_ground(pwpp_handle *h, const float *xyz /* (m,3) row-major */, const int32_t *frame /* m entries, or NULL: frame 0 */,
                               int64_t m, int mem, pwpp_ground_sample *out);
/* The same as an image: cell (ix, iy) of a frame is the query of its centre,
 *     cx = (float)(x0 + (ix + 0.5) * cell),   cy = (float)(y0 + (iy + 0.5) * cell)     evaluated in double,
 * height[f][iy][ix] that query's ground_z and patch[f][iy][ix] its row (patch may be NULL), for the frames frame_first ..
 * frame_first + frames - 1 of the last call.  With PWPP_GRID_GROUND_ONLY the cells whose patch was decided NOT_UPRIGHT, HEADING or
 * TGR_REJECT get a NaN height; their row is still reported.  PWPP_E_ARG: a null grid or height, nx or ny < 1, a cell that is not
 * finite and positive, a frame range outside the last call, nx * ny * frames beyond 2^31. */
typedef struct pwpp_ground_grid { double x0, y0, cell; int32_t nx, ny; int32_t flags; int32_t pad_; } pwpp_ground_grid;
enum { PWPP_GRID_GROUND_ONLY = 1 };
PWPP_API int pwpp_rasterize_ground(pwpp_handle *h, const pwpp_ground_grid *g, int frame_first, int frames, int mem,
                                   float *height /* [frames][ny][nx] */, int32_t *patch /* same shape, may be NULL */);

/* ---- the non-ground points as an obstacle grid (pwpp_rasterize_obstacles) --------------------------------------------------------
 * The other half of a 2.5-D map on the grid of pwpp_rasterize_ground: per cell how many non-ground returns, how tall the tallest,
 * and how many nobody can vouch for -- what a costmap, an occupancy grid or a BEV detector builds next, without the lists or the
 * coordinates of a batch leaving the device.
 *   When, mem Exactly as pwpp_rasterize_ground: answers from the handle's LAST estimate call of any kind (a pipe's handles
 *             included), enters like the getters (the call in flight lands first, a frame that awaits the fix-up or a redo is
 *             finished first), PWPP_E_STATE before any call and after pwpp_trim_workspace.  PWPP_MEM_HOST: the images are host
 *             memory, staged through the ground queries' buffer; synchronous.  PWPP_MEM_DEVICE: device memory (4-byte aligned, no
 *             more), enqueued on the handle's stream, complete after pwpp_synchronize.  PWPP_MEM_HOST_PINNED: PWPP_E_ARG.  A pure
 *             read: no result, state or timing of the estimate path changes, and nothing is allocated beyond what the ground
 *             queries hold.
 *   points    The points the frame's non-ground index list names (n_nonground entries, in whatever output order the handle has),
 *             read from the frame's INPUT as the pipeline reads it: with input transforms set, the transformed coordinates.  The
 *             lifetime rule of pwpp_get_nonground_xyz applies: after a PWPP_MEM_DEVICE estimate call the caller's buffer must still
 *             hold the frame when this call runs.
 *   reference The sample pwpp_query_ground gives for the point's own (x, y, z): position-query semantics, unchanged.  Consequence:
 *             an RNR point is in the non-ground list and queries into its bin's patch with a large negative distance (RNR only
 *             takes points more than 0.8 m below the sensor's ground level): a band with h_min above about -0.8 m leaves it out.
 *             A point has NO reference where that sample has patch == -1 -- outside (min_range, max_range], a bin with fewer than
 *             num_min_pts points, a non-finite x or y -- and, with PWPP_GRID_GROUND_ONLY in g->flags, also where its patch was
 *             decided NOT_UPRIGHT, HEADING or TGR_REJECT: the three decisions the ground raster blanks.
 *   height    hgt = that sample's distance: the point-planes formula against the patch's REPORTED plane, the number
 *             pwpp_get_point_distances has for a point that owns its patch.  A point is COUNTED iff it has a reference and
 *             h_min <= hgt && hgt <= h_max as float comparisons (a NaN height is not counted).  Infinite bounds are legal.
 *   cell      In double on the float coordinates, one subtraction and one IEEE division each, no reciprocal, no FMA:
 *                 u = ((double)x - x0) / cell,   ix = (int)floor(u),   kept iff 0 <= u && u < nx;     v, iy alike with y, y0, ny
 *             A point outside the grid, or whose u or v is a NaN, touches no image.
 *   images    count[f][iy][ix]  the counted points of the cell;
 *             unref[f][iy][ix]  the points of the cell without a reference (may be NULL);
 *             top[f][iy][ix]    the largest hgt among the counted points, in the total order in which -0.0 < +0.0; the quiet NaN
 *                               where count is 0 (may be NULL);
 *             for the frames frame_first .. frame_first + frames - 1 of the last call.  Integer adds and an integer-keyed maximum
 *             only: all three are functions of the input alone -- bit-reproducible from call to call, independent of the output
 *             order, the schedule and the memory kind of the estimate call.
 *   errors    PWPP_E_ARG: everything pwpp_rasterize_ground rejects of a grid and a frame range (nx * ny * frames beyond 2^31
 *             included), a null count, flags other than 0 or PWPP_GRID_GROUND_ONLY, a NaN h_min or h_max, h_min > h_max. */
#define PWPP_HAS_OBSTACLE_GRID 1
PWPP_API int pwpp_rasterize_obstacles(pwpp_handle *h, const pwpp_ground_grid *g, float h_min, float h_max,
                                      int frame_first, int frames, int mem,
                                      int32_t *count /* [frames][ny][nx] */,
                                      float   *top   /* same shape, may be NULL */,
                                      int32_t *unref /* same shape, may be NULL */);

/* ---- the occupied cells of an obstacle grid as connected clusters (pwpp_label_grid, pwpp_label_obstacles) ------------------------
 * The last piece of the 2.5-D map: which cells of the obstacle grid belong together.  Connected-component labelling of the count
 * image on the device -- the step before tracking, boxes or a per-object costmap -- without an image per frame leaving the
 * device, and for pwpp_label_obstacles without the caller restating the cell arithmetic to map points to cells.
 *   occupied  A cell is occupied iff count >= min_count; min_count >= 1.
 *   cluster   A maximal set of occupied cells of ONE frame that are connected through edge neighbours (connectivity 4) or edge
 *             and corner neighbours (connectivity 8).  Frames never connect.
 *   label     label[f][iy][ix] is -1 for an unoccupied cell, else the RANK of the cell's cluster among the frame's clusters in
 *             ascending first_cell: 0, 1, 2, ...  That rank is the cluster's row in the frame's part of `clusters`.  The ranks
 *             are complete also when the frame has more clusters than max_clusters.
 *   clusters  Row r of frame f (clusters[f * max_clusters + r]) is the cluster of rank r, for the first min(n, max_clusters)
 *             ranks; rows beyond the frame's n are unspecified.  n_clusters[f] is the frame's TRUE number of clusters, also when
 *             it exceeds max_clusters.  Every sum is an integer sum and the maximum is taken on the integer key of
 *             pwpp_rasterize_obstacles: label image, table and counts are functions of the count and top images alone --
 *             bit-reproducible from call to call, and in pwpp_label_obstacles independent of the output order, the schedule and
 *             the memory kind of the estimate call.
 *   label_obstacles   count and top are exactly the images pwpp_rasterize_obstacles(g, h_min, h_max, ...) gives for the frame
 *             range, written for the caller where asked for and kept in the handle's cluster buffer otherwise; label, clusters and
 *             n_clusters are exactly what pwpp_label_grid gives for those two images.  When, mem, the grid's flags, the lifetime
 *             rule of the INPUT and the errors are those of pwpp_rasterize_obstacles.
 *   point_cluster     One int32 per point of the frame range, in cloud order: frame f starts at frame_base[f] -
 *             frame_base[frame_first], frame_base as in pwpp_get_device_view.  A point's value is the label of its cell iff it is
 *             a COUNTED point of the obstacle grid (named by the non-ground list, inside the grid, has a reference, height in the
 *             band: pwpp_rasterize_obstacles' rules, evaluated by the same device function).  Every other point gets -1: ground,
 *             unclassified, without a reference, out of the band, out of the grid, or in a cell below min_count.
 *   mem       PWPP_MEM_HOST: every array is host memory, staged through the handle's cluster buffer; synchronous.
 *             PWPP_MEM_DEVICE: device memory, 4-byte aligned and no more -- except `clusters`, which must be 8-byte aligned --
 *             enqueued on the handle's stream, complete after pwpp_synchronize.  PWPP_MEM_HOST_PINNED: PWPP_E_ARG.
 *   errors    PWPP_E_ARG: a null handle, label or (pwpp_label_grid) count; nx, ny or frames < 1; nx * ny beyond 2^31 - 1 or
 *             nx * ny * frames beyond 2^31; min_count < 1; a connectivity other than 4 or 8; max_clusters < 0; max_clusters > 0
 *             with a null clusters; for pwpp_label_obstacles everything pwpp_rasterize_obstacles rejects.  Null arguments are
 *             named before the device is touched.  pwpp_label_obstacles before any estimate call: PWPP_E_STATE.
 *   buffers   One cluster buffer per handle holds the working image (a root's rank inside its counting unit), the per-unit root
 *             counts, and the images, table and ids a call stages or keeps.  It is allocated on first use, counted by
 *             pwpp_get_workspace_bytes and freed by pwpp_trim_workspace.  pwpp_label_grid needs a handle for its stream and this
 *             buffer only: it enters like a getter (the call in flight lands first) and works before any estimate call.
 * With neither function called nothing is allocated or launched, and no result, state or timing of the estimate path changes. */
#define PWPP_HAS_OBSTACLE_CLUSTERS 1
typedef struct pwpp_obstacle_cluster {   /* 48 bytes */
    int32_t first_cell;                  /* iy * nx + ix of the cluster's smallest cell in row-major order: its canonical name */
    int32_t cells;                       /* occupied cells */
    int32_t points;                      /* sum of count over them */
    int32_t ix_min, ix_max, iy_min, iy_max;
    float   top;                         /* largest top over them, in the order of pwpp_rasterize_obstacles (-0.0 < +0.0); NaN when no top image */
    int64_t sum_ix, sum_iy;              /* sum of count * ix, count * iy: the point-weighted centroid is x0 + (sum_ix / points + 0.5) * cell */
} pwpp_obstacle_cluster;
/* any occupancy image: needs a handle (stream, buffers), no estimate call */
PWPP_API int pwpp_label_grid(pwpp_handle *h, int nx, int ny, int frames, int mem,
                             const int32_t *count, const float *top /* may be NULL */,
                             int min_count, int connectivity /* 4 or 8 */,
                             int32_t *label /* [frames][ny][nx] */,
                             pwpp_obstacle_cluster *clusters /* [frames][max_clusters], may be NULL */,
                             int32_t *n_clusters /* [frames], may be NULL */, int max_clusters);
/* rasterize + label for frames of the LAST estimate call, one call */
PWPP_API int pwpp_label_obstacles(pwpp_handle *h, const pwpp_ground_grid *g, float h_min, float h_max,
                                  int min_count, int connectivity, int frame_first, int frames, int mem,
                                  int32_t *label, int32_t *count /* may be NULL */, float *top /* may be NULL */,
                                  pwpp_obstacle_cluster *clusters, int32_t *n_clusters, int max_clusters,
                                  int32_t *point_cluster /* may be NULL */);

/* ---- every cluster of the obstacle grid as an oriented box (pwpp_box_obstacles, pwpp_box_points) ----------------------------------
 * The step from cells to objects: the COUNTED points of every label of a label image reduced to a centre and a heading in metres,
 * a length and a width, the spread along and across, and the vertical extent -- what a tracker, a box publisher or a costmap
 * inflater takes -- without point_cluster and the coordinates of a batch leaving the device.
 *   counted   The points pwpp_rasterize_obstacles(g, h_min, h_max, ...) counts (one device function decides it for all of them).
 *   row       A counted point of frame f in cell c belongs to row label[f][c]; it contributes to boxes[f * max_boxes + row] iff
 *             0 <= row < max_boxes, every other value (-1, a rank beyond the table) is skipped.  The label image is the
 *             caller's: what pwpp_label_obstacles wrote for the same grid and band, or an edited one -- clusters merged, dropped,
 *             renumbered.  No min_count and no connectivity enters here.  It is not written.
 *   arithmetic   Part of the contract; only + - * / sqrt, no FMA.  With dx = (double)x - x0, dy = (double)y - y0 (the doubles the
 *             cell arithmetic starts from):
 *             1  qx = llrint(dx * 1024), qy alike (ties to even); per row the 64-bit integer sums N, Sx, Sy, Sxx, Sxy, Syy.
 *             2  A = N Sxx - Sx Sx, B = N Sxy - Sx Sy, C = N Syy - Sy Sy in 128-bit integers; each rounded ONCE to a double a, b, c.
 *             3  d = (a - c) * 0.5; r = sqrt(d*d + b*b); (vx, vy) = d >= 0 ? (d + r, b) : (b, r - d); n = sqrt(vx*vx + vy*vy);
 *                the axis is (vx / n, vy / n), negated when ux < 0 or (ux == 0 and uy < 0) -- or (1, 0) when n is not finite and
 *                positive (one point, coincident points, an isotropic set).  ax = (float)ux, ay = (float)uy.
 *             4  m = (a + c) * 0.5; sigma_long = (float)(sqrt(m + r) / ((double)N * 1024)), sigma_short alike from max(m - r, 0);
 *                mean_x = (float)(x0 + ((double)Sx / (double)N) / 1024), mean_y alike.
 *             5  per point p = (float)(dx * (double)ax + dy * (double)ay), q = (float)(dy * (double)ax - dx * (double)ay): against
 *                the FLOAT axis, so the box is a rectangle in the reported frame.  Minima and maxima of p, q, the height over
 *                ground and z on the integer key of pwpp_rasterize_obstacles (-0.0 < +0.0).  length = (float)((double)pmax -
 *                (double)pmin), width alike from q; pc = ((double)pmin + (double)pmax) * 0.5, qc alike;
 *                cx = (float)(x0 + (pc * (double)ax - qc * (double)ay)), cy = (float)(y0 + (pc * (double)ay + qc * (double)ax)).
 *             Integer sums, minima and maxima commute: every field is a function of the input, the grid, the band and the label
 *             image alone -- the same bytes for every output order, schedule, memory kind and value of the option "boxes_path".
 *   extent    nx * cell <= 1024 and ny * cell <= 1024 (in double): then q <= 2^20 + 1 and the sums of a frame's 2^22 points stay
 *             below 2^63.  frames * max_boxes <= 2^24.
 *   rows      A row no counted point named: points 0, every float the quiet NaN (0x7fc00000).  For the rows of a
 *             pwpp_label_obstacles table `points` equals the cluster row's points and h_max has the bits of its top.
 *   when, mem, errors   Those of pwpp_label_obstacles: frames of the LAST estimate call, the lifetime rule of the input, PWPP_E_STATE
 *             before any estimate call.  PWPP_MEM_HOST: label and boxes are host memory, staged through the handle's cluster
 *             buffer; synchronous.  PWPP_MEM_DEVICE: device memory, 4-byte aligned and no more, enqueued on the handle's stream,
 *             complete after pwpp_synchronize; boxes is also the kernels' scratch between the passes.  PWPP_MEM_HOST_PINNED,
 *             a null handle, grid, label or boxes, max_boxes < 1, an extent beyond 1024 m: PWPP_E_ARG, named before the device
 *             is touched.  The accumulators (80 bytes per row) live in the cluster buffer: allocated on first use, counted by
 *             pwpp_get_workspace_bytes, freed by pwpp_trim_workspace.
 *   box_points   Host only, no handle, no device: the same rows for a caller's own points, compiled from the same functions as
 *             the kernels.  Row and height over ground of every point are the caller's, z is xyz[:, 2].  Skipped: a row outside
 *             [0, max_boxes), a NaN hgt, a point outside the grid (the cell rule of pwpp_rasterize_ground).  m <= 2^22.
 * With neither function called nothing is allocated or launched, and no result, state or timing of the estimate path changes. */
#define PWPP_HAS_OBSTACLE_BOXES 1
typedef struct pwpp_obstacle_box {      /* 64 bytes, 4-byte aligned fields only */
    int32_t points;                     /* counted points that named this row; 0: every float below is the quiet NaN */
    int32_t pad_;                       /* 0 */
    float mean_x, mean_y;               /* point mean, from the 1/1024 m moments */
    float cx, cy;                       /* centre of the box */
    float ax, ay;                       /* unit vector of the principal axis; ax > 0, or ax == 0 and ay > 0 */
    float length, width;                /* extent along the axis / across it (length is NOT forced >= width) */
    float sigma_long, sigma_short;      /* standard deviations along / across, metres */
    float h_min, h_max;                 /* lowest / largest height over ground (the obstacle grid's height) */
    float z_min, z_max;                 /* lowest / largest z as the pipeline read it (transformed, if transforms are set) */
} pwpp_obstacle_box;
/* rows for frames of the LAST estimate call, from a label image on the obstacle grid g */
PWPP_API int pwpp_box_obstacles(pwpp_handle *h, const pwpp_ground_grid *g, float h_min, float h_max,
                                int frame_first, int frames, int mem,
                                const int32_t *label /* [frames][ny][nx] */,
                                pwpp_obstacle_box *boxes /* [frames][max_boxes] */, int max_boxes);
/* host only, no device: the same arithmetic for a caller's own points */
PWPP_API int pwpp_box_points(const pwpp_ground_grid *g, const float *xyz /* (m,3) */, const float *hgt /* m */,
                             const int32_t *row /* m */, int64_t m, pwpp_obstacle_box *boxes, int max_boxes);

/* ---- the outline of every cluster: its convex hull and its tightest rectangle (pwpp_hull_obstacles, pwpp_hull_points) --------------
 * The box of pwpp_box_obstacles stands on the principal axis of the points, which is the wrong axis for the clusters a lidar sees
 * most: a car seen from a corner is an L whose principal axis is its diagonal, a wall with one return at its end is swung round by
 * it.  Here every row gets the exact convex hull of its counted points on the 1/1024 m grid of the boxes, and from the hull the
 * enclosing rectangle of least area, chosen by exact integer comparison -- without point_cluster and the coordinates of a batch
 * leaving the device.  Integers first, six floats derived once.
 *   points    Exactly the counted points of pwpp_box_obstacles (one device function decides), the same rule of a row: a point of
 *             frame f in cell c belongs to row label[f][c] iff 0 <= row < max_hulls.  A point is the integer pair (qx, qy) =
 *             (llrint(dx * 1024), llrint(dy * 1024)) of the boxes' step 1, 0 <= q <= 2^20 + 1; the extent limit of the boxes applies
 *             (nx * cell <= 1024, ny * cell <= 1024).  A row's input is the SET of its distinct pairs: duplicates count once for
 *             the hull and every time for `points`.
 *   hull      The vertices of the strict convex hull.  cross(a, b, c) = (bx-ax)*(cy-ay) - (by-ay)*(cx-ax) in int64 (|cross| < 2^43,
 *             exact).  Consecutive vertices a, b, c have cross > 0 (counter-clockwise, y up); no vertex lies on the segment between
 *             two others.  The list starts at the vertex with the smallest (qy, qx).  One distinct point: 1 vertex.  A collinear set:
 *             2 vertices, the smallest then the largest under (qy, qx).  n_vertices is the TRUE count; stored = min(n_vertices,
 *             max_vertices); the first `stored` vertices are written to vertices[f][row][k] = {qx, qy}, entries from `stored` on are
 *             unspecified.  area2 = the shoelace sum over all n_vertices edges, twice the area in (1/1024 m)^2 -- exact also for
 *             a truncated list.  qx_min .. qy_max: the bounds of the row's points (= of its vertices).
 *   rectangle Defined iff 1 <= n_vertices <= max_vertices.  For edge i, from vertex i to vertex i + 1 mod n, let e = (ex, ey) be its
 *             vector, negated when ex < 0 or (ex == 0 and ey < 0); e = (1, 0) for a row of 1 vertex.  Over all vertices v: p = ex*vx +
 *             ey*vy, q = ex*vy - ey*vx in int64; W = pmax - pmin, H = qmax - qmin, L2 = ex*ex + ey*ey.  Edge i is better than edge j iff
 *             W_i*H_i*L2_j < W_j*H_j*L2_i in unsigned 128-bit integers: with diam the diameter of the set, diam^2 <= 2 (2^20 + 1)^2 <
 *             2^41 + 2^23, W*H <= diam^2 * L2 and L2 <= diam^2, so both sides are at most diam^6 < 2^124.  Ties go to the lower i;
 *             rect_edge is that i.  Floats as for the boxes, only + - * / sqrt, no FMA, every integer exact in a double or rounded
 *             to one ONCE: L = sqrt((double)L2); ax = (float)((double)ex / L), ay alike; length = (float)(((double)W / L) / 1024),
 *             width alike from H; U = (pmin+pmax)*ex - (qmin+qmax)*ey and V = (pmin+pmax)*ey + (qmin+qmax)*ex in 128-bit integers,
 *             each rounded once to a double u, v; cx = (float)(x0 + (u / (2.0 * (double)L2)) / 1024), cy alike from v and y0.
 *             length is NOT forced >= width.
 *   rows      A row no counted point named: every integer 0 except rect_edge = -1, every float the quiet NaN (0x7fc00000).  A
 *             truncated row (n_vertices > max_vertices): the integers filled, rect_edge = -1, the six floats NaN.
 *   invariants   Every counted point of a row has cross >= 0 against every hull edge.  Where both are defined, the rectangle is
 *             no larger than the box of the same row: the exact rational W*H/L2 of the chosen edge is <= the area of the
 *             rectangle that encloses the row's integer points along the box's float axis (ax, ay), (pmax - pmin)(qmax - qmin) /
 *             (ax^2 + ay^2) in exact arithmetic -- the least enclosing rectangle has a side on a hull edge.  The floats length *
 *             width of the two rows differ from those rationals by their own roundings only.  The bytes depend on the input, the
 *             grid, the band and the label image alone: not on output order, schedule, memory kind or the option "hulls_path".
 *   when, mem, lifetime, errors   Those of pwpp_box_obstacles.  PWPP_MEM_DEVICE: hulls 8-byte aligned (like pwpp_obstacle_cluster), label and
 *             vertices 4-byte.  PWPP_E_ARG, named before the device is touched, also for max_hulls < 1, max_vertices outside 1 ..
 *             1024, frames * max_hulls > 2^24, frames * max_hulls * max_vertices > 2^28.  vertices may be NULL: the rows are the
 *             same bytes.  In the cluster buffer (allocated on first use, counted by pwpp_get_workspace_bytes, freed by
 *             pwpp_trim_workspace): 80 bytes of accumulators per row, and the candidate arena -- the points that lie not
 *             strictly inside the octagon of their row's eight extreme points, 8 bytes each, laid out per row by an exclusive scan
 *             of the rows' point counts: 8 * frames * (the longest non-ground list of the frame range) bytes.
 *   hull_points   Host only, no handle, no device: the same rows for a caller's own points, compiled from the same functions as the
 *             kernels; hulls[max_hulls], vertices[max_hulls][max_vertices][2] or NULL.  Skipped: a row outside [0, max_hulls), a
 *             point outside the grid (the cell rule of pwpp_box_points), a NaN z (its height over ground is a NaN: never counted).
 *             m <= 2^22.
 *   hull_vertex_xy   Host only: out[0] = (double)(x0 + q[0] / 1024.0), out[1] = (double)(y0 + q[1] / 1024.0).
 * With none of the three called nothing is allocated or launched, and no result, state or timing of any other entry point changes. */
#define PWPP_HAS_OBSTACLE_HULLS 1
#define PWPP_HULL_VERTICES_MAX 1024
typedef struct pwpp_obstacle_hull {     /* 64 bytes, 8-byte aligned */
    int32_t points;                     /* counted points that named this row, duplicates included; 0: the empty row */
    int32_t n_vertices;                 /* vertices of the strict hull: the true count */
    int32_t stored;                     /* min(n_vertices, max_vertices): how many of them the list holds */
    int32_t rect_edge;                  /* the edge the rectangle stands on; -1: no rectangle (empty or truncated row) */
    int64_t area2;                      /* twice the hull's area, (1/1024 m)^2 */
    int32_t qx_min, qx_max, qy_min, qy_max; /* bounds of the points on the 1/1024 m grid */
    float cx, cy;                       /* centre of the rectangle, metres */
    float ax, ay;                       /* unit vector of the chosen edge; ax > 0, or ax == 0 and ay > 0 */
    float length, width;                /* extent along the edge / across it, metres */
} pwpp_obstacle_hull;
PWPP_API int pwpp_hull_obstacles(pwpp_handle *h, const pwpp_ground_grid *g, float h_min, float h_max,
                                 int frame_first, int frames, int mem,
                                 const int32_t *label /* [frames][ny][nx] */,
                                 pwpp_obstacle_hull *hulls /* [frames][max_hulls] */, int max_hulls,
                                 int32_t *vertices /* [frames][max_hulls][max_vertices][2], may be NULL */, int max_vertices);
PWPP_API int pwpp_hull_points(const pwpp_ground_grid *g, const float *xyz /* (m,3) */, const int32_t *row /* m */, int64_t m,
                              pwpp_obstacle_hull *hulls, int max_hulls, int32_t *vertices /* may be NULL */, int max_vertices);
PWPP_API int pwpp_hull_vertex_xy(const pwpp_ground_grid *g, const int32_t *q /* {qx, qy} */, double *out /* {x, y} */);

/* ---- the distance of every cell to the nearest occupied cell (pwpp_distance_grid, pwpp_distance_obstacles) ------------------------
 * What a costmap, a planner and a collision check start from: for every cell of an obstacle grid, occupied or free, how far the
 * nearest occupied cell is and which one it is -- an exact Euclidean distance transform on the device, each frame on its own,
 * without a count image per frame leaving the device for a CPU transform.
 *   occupied  A cell is occupied iff count >= min_count; min_count >= 1 (the rule of pwpp_label_grid).
 *   dist2     dist2[f][iy][ix] = the minimum of (ix - jx)^2 + (iy - jy)^2 over the occupied cells (jx, jy) of the same frame, an
 *             exact integer: 0 on an occupied cell, PWPP_DIST_BEYOND when the frame has no occupied cell.
 *   nearest   nearest[f][iy][ix] = jy * nx + jx of the cell that attains the minimum, the SMALLEST such index among several; -1
 *             where dist2 is PWPP_DIST_BEYOND.  Consequence: label[f].flat[nearest] is the nearest cluster of every cell.
 *   metres    metres[f][iy][ix] = (float)(sqrt((double)dist2) * cell): one correctly rounded square root, one multiply in double,
 *             one rounding to float; +inf where dist2 is PWPP_DIST_BEYOND.  pwpp_distance_obstacles uses g->cell; `cell` is read
 *             only when metres != NULL.
 *   max_dist  Cells, 0 .. 46340; 0: unlimited.  With max_dist > 0 every cell whose TRUE dist2 exceeds max_dist^2 reports
 *             PWPP_DIST_BEYOND / -1 / +inf, and every other cell exactly what the unlimited call reports: it lets the kernels
 *             bound their search (an inflation radius is a few metres), it is not an approximation.
 *   Frames never influence each other.  All three images are functions of the count image alone: the same bytes for every call,
 *   mem, alignment, max_dist window strategy and value of the option "distance_path".
 *   distance_obstacles   count is exactly the image pwpp_rasterize_obstacles(g, h_min, h_max, ...) gives for the frame range,
 *             written for the caller where asked for and kept in the handle's cluster buffer otherwise; the other images are
 *             exactly what pwpp_distance_grid gives for it.  When, mem, the grid's flags, the lifetime rule of the INPUT and the
 *             errors are those of pwpp_label_obstacles.
 *   mem       PWPP_MEM_HOST: every array is host memory, staged through the handle's cluster buffer; synchronous.
 *             PWPP_MEM_DEVICE: device memory, 4-byte aligned and no more, enqueued on the handle's stream, complete after
 *             pwpp_synchronize.  PWPP_MEM_HOST_PINNED: PWPP_E_ARG.
 *   errors    PWPP_E_ARG, named before the device is touched: a null handle, (pwpp_distance_grid) count, dist2 or grid; nx, ny or
 *             frames < 1; nx or ny > 32768 (the largest possible dist2, 2 * 32767^2, stays below PWPP_DIST_BEYOND); nx * ny *
 *             frames beyond 2^31; min_count < 1; max_dist outside 0 .. 46340; a non-null metres with a cell that is not finite
 *             and positive; for pwpp_distance_obstacles everything pwpp_rasterize_obstacles rejects.  pwpp_distance_obstacles
 *             before any estimate call: PWPP_E_STATE.
 *   buffers   The kernels' working image lives in the cluster buffer: one int32 per cell, the nearest occupied column of the
 *             cell's own row.  Allocated on first use, counted by pwpp_get_workspace_bytes, freed by pwpp_trim_workspace.
 *             pwpp_distance_grid needs a handle for its stream and this buffer only, like pwpp_label_grid.
 * With neither function called nothing is allocated or launched, and no result, state or timing of the estimate path changes. */
#define PWPP_HAS_OBSTACLE_DISTANCE 1
#define PWPP_DIST_BEYOND 0x7fffffff
/* any occupancy image: needs a handle (stream, buffer), no estimate call -- like pwpp_label_grid */
PWPP_API int pwpp_distance_grid(pwpp_handle *h, int nx, int ny, int frames, int mem,
                                const int32_t *count /* [frames][ny][nx] */, int min_count,
                                int max_dist /* cells; 0: unlimited */, double cell /* metres per cell; read only when metres != NULL */,
                                int32_t *dist2 /* [frames][ny][nx] */, int32_t *nearest /* same shape, may be NULL */,
                                float *metres /* same shape, may be NULL */);
/* rasterize + distance for frames of the LAST estimate call, one call -- like pwpp_label_obstacles */
PWPP_API int pwpp_distance_obstacles(pwpp_handle *h, const pwpp_ground_grid *g, float h_min, float h_max,
                                     int min_count, int max_dist, int frame_first, int frames, int mem,
                                     int32_t *dist2, int32_t *nearest /* may be NULL */, float *metres /* may be NULL */,
                                     int32_t *count /* may be NULL: kept in the handle's buffer */);

/* ---- line-of-sight free space on the obstacle grid (pwpp_visibility_grid, pwpp_visibility_obstacles) ------------------------------
 * What separates a cell that holds no obstacle because it was SEEN to be empty from one that holds none because something hides
 * it from the sensor: for every cell of an occupancy image the first occupied cell on the digital line from the sensor's cell,
 * and from it the tri-state byte of a nav_msgs/OccupancyGrid -- on the device, each frame on its own, all integer arithmetic.
 * THIS IS 2-D LINE OF SIGHT ON A 2.5-D MAP: a free cell behind a low obstacle that the sensor saw OVER is reported unknown.
 *   occupied  A cell is occupied iff count >= min_count; min_count >= 1 (the rule of pwpp_label_grid).
 *   origin    One sensor cell o = (ox, oy) per frame, inside the image.  n_origins == 1: that origin for every frame; n_origins ==
 *             frames: entry i for frame frame_first + i; any other number: PWPP_E_ARG.  The array is HOST memory in both mem kinds
 *             and is copied at the call (as pwpp_set_input_transforms copies T): the caller may free it on return.
 *             pwpp_visibility_obstacles takes positions in metres in the model's frame -- normally {0, 0}; with input transforms
 *             set, the t of the transform -- and turns them into cells by the cell rule of pwpp_rasterize_obstacles, in double:
 *             u = (x - x0) / cell, ox = (int)floor(u).  A position that is not finite or falls outside the grid: PWPP_E_ARG, naming
 *             the entry.
 *   line      For the cell c = (cx, cy): dx = cx - ox, dy = cy - oy, n = max(|dx|, |dy|); P_0 = o and for k = 1 .. n
 *             P_k = (ox + sgn(dx) * ((2k|dx| + n) / (2n)), oy + sgn(dy) * ((2k|dy| + n) / (2n))), the divisions rounding down.
 *             P_n = c; consecutive points differ by at most 1 in each coordinate.
 *   first     Walk k = 1 .. n; at each step, in this order: (a) if both coordinates changed from P_{k-1} to P_k, take
 *             A = (x_{k-1}, y_k) and B = (x_k, y_{k-1}); both occupied: the line is blocked, first = the smaller of their indices
 *             (jy * nx + jx), stop -- a line does not squeeze diagonally between two occupied cells, so a wall that is only
 *             8-connected is opaque; (b) if P_k is occupied: first = its index, stop.  Nothing found: PWPP_VIS_NONE.  n == 0: the
 *             cell's own index if it is occupied, else PWPP_VIS_NONE.  The origin's cell never blocks another cell (k starts at
 *             1): it holds the vehicle's own returns.  So first == own index: a seen surface; first == PWPP_VIS_NONE: seen and
 *             free; anything else: hidden, and label[f].flat[first] is the cluster that hides it.
 *   max_range Cells, Chebyshev, 0 .. 32768; 0: unlimited.  A cell with n > max_range reports PWPP_VIS_BEYOND, every other cell
 *             exactly what the unlimited call reports (its walk only passes cells with a smaller n): it bounds the work, it is
 *             not an approximation.
 *   occupancy PWPP_OCC_OCCUPIED where the cell is occupied, hidden or not (it holds returns: it was seen in 3-D); otherwise
 *             PWPP_OCC_FREE where first == PWPP_VIS_NONE; PWPP_OCC_UNKNOWN in all other cases, hidden or beyond range.
 *   Frames never influence each other.  Both images are functions of the count image, the origins, min_count and max_range alone:
 *   the same bytes for every call, mem, alignment and value of the option "visibility_path".
 *   visibility_obstacles   count is exactly the image pwpp_rasterize_obstacles(g, h_min, h_max, ...) gives for the frame range,
 *             written for the caller where asked for and kept in the handle's cluster buffer otherwise; the other images are
 *             exactly what pwpp_visibility_grid gives for it.  When, mem, the grid's flags, the lifetime rule of the INPUT and the
 *             errors are those of pwpp_distance_obstacles.
 *   mem       PWPP_MEM_HOST: every image is host memory, staged through the handle's cluster buffer; synchronous.
 *             PWPP_MEM_DEVICE: device memory -- first and count 4-byte aligned and no more, occupancy byte aligned -- enqueued on
 *             the handle's stream, complete after pwpp_synchronize.  PWPP_MEM_HOST_PINNED: PWPP_E_ARG.
 *   errors    PWPP_E_ARG, named before the device is touched, in this order: a null handle, count, first, origin or grid; nx, ny
 *             or frames < 1; nx or ny > 32768; nx * ny * frames beyond 2^31; min_count < 1; max_range outside 0 .. 32768; the
 *             number of origins; an origin outside the image; mem.  For pwpp_visibility_obstacles everything
 *             pwpp_rasterize_obstacles rejects; before any estimate call: PWPP_E_STATE.
 *   buffers   The kernels' working image lives in the cluster buffer: one BIT per cell, rows padded to 32 (8 KiB for 256 x 256
 *             cells), and the origins where there is one per frame.  Allocated on first use, counted by pwpp_get_workspace_bytes,
 *             freed by pwpp_trim_workspace.  pwpp_visibility_grid needs a handle for its stream and this buffer only.
 * With neither function called nothing is allocated or launched, and no result, state or timing of the estimate path changes. */
#define PWPP_HAS_OBSTACLE_VISIBILITY 1
#define PWPP_VIS_NONE   (-1)   /* nothing on the line: the cell is seen */
#define PWPP_VIS_BEYOND (-2)   /* further than max_range: not examined */
enum { PWPP_OCC_FREE = 0, PWPP_OCC_OCCUPIED = 100, PWPP_OCC_UNKNOWN = -1 };   /* nav_msgs/OccupancyGrid values */

/* any occupancy image: needs a handle (stream, buffer), no estimate call -- like pwpp_distance_grid */
PWPP_API int pwpp_visibility_grid(pwpp_handle *h, int nx, int ny, int frames, int mem,
                                  const int32_t *count /* [frames][ny][nx] */, int min_count,
                                  const int32_t *origin /* HOST memory, n_origins x {ox, oy} cells */, int n_origins,
                                  int max_range /* cells, Chebyshev; 0: unlimited */,
                                  int32_t *first /* [frames][ny][nx] */, int8_t *occupancy /* same shape, may be NULL */);
/* rasterize + visibility for frames of the LAST estimate call, one call -- like pwpp_distance_obstacles */
PWPP_API int pwpp_visibility_obstacles(pwpp_handle *h, const pwpp_ground_grid *g, float h_min, float h_max,
                                       int min_count, const double *origin_xy /* HOST, n_origins x {x, y} metres */, int n_origins,
                                       int max_range, int frame_first, int frames, int mem,
                                       int32_t *first, int8_t *occupancy /* may be NULL */, int32_t *count /* may be NULL: kept */);

/* ---- persistent log-odds maps: per-frame occupancy fused over time (pwpp_fuse_grid, pwpp_fuse_obstacles) -------------------------
 * One scan sees little: the occupancy byte of the visibility says "unknown" for most cells of a frame.  A map a planner can drive
 * on accumulates the scans in a FIXED frame, given the vehicle's pose: the log-odds update of every occupancy-grid mapper -- here
 * on the device, with integer state and a fixed arithmetic, so that the fused map is a function of its inputs alone and bit-
 * reproducible.  The maps are the caller's arrays, like every other image; a handle holds nothing of them between calls.
 * All n_maps maps share the geometry and parameters of *m.  Below (X0, Y0, CELL, NX, NY) are m's fields, (x0, y0, cell, nx, ny) g's.
 *   pose      Map-from-frame, six doubles {a, b, tx, c, d, ty}: a frame position (x, y) lies at (a x + b y + tx, c x + d y + ty)
 *             in the map's frame.  A matrix, not an angle: no sin or cos enters the contract.  HOST memory in both mem kinds,
 *             copied at the call (like the origins of the visibility).  n_poses == 1: that pose for every frame; n_poses ==
 *             frames: entry i for frame i; any other number: PWPP_E_ARG.  Nothing checks orthonormality: the inverse used is the
 *             TRANSPOSE (below), exact for a rotation; for anything else -- a mirror, a scale -- the formula is the definition.  A
 *             pose that is not finite is no error: its samples are outside, the frame observes nothing.
 *   samples   The operator is a gather: a map cell asks the frames, a frame cell never writes.  The map cell (jx, jy) is sampled at
 *             the centres of its four quadrants, q = (qx, qy) in {0, 1}^2, all in double, every product, sum and quotient rounded
 *             on its own (no FMA):
 *                 mx = X0 + ((double)jx + (0.25 + 0.5 * qx)) * CELL          my alike with jy, qy, Y0
 *                 dx = mx - tx;  dy = my - ty
 *                 fx = a * dx + c * dy;   fy = b * dx + d * dy
 *                 u = (fx - x0) / cell;  ix = (int)floor(u), inside iff 0 <= u && u < nx      v, iy alike with fy, y0, ny
 *             (the cell rule of pwpp_rasterize_obstacles).  A sample outside the frame image, or whose u or v is a NaN, reads
 *             PWPP_OCC_UNKNOWN; every other sample reads occupancy[f][iy][ix].
 *             Why four samples and not the centre: with equal cell sizes and a yaw of 45 degrees, 17.7 % of the frame's cells lie
 *             under no map cell's centre (13 % at 30 degrees) -- a thin obstacle would vanish from a frame.  The quadrant centres
 *             form a lattice of spacing CELL / 2 with covering radius 0.354 CELL, less than the inscribed radius 0.5 cell of a
 *             frame cell whenever CELL <= cell.  THE GUARANTEE: under a rigid pose with CELL <= cell, every occupied frame cell
 *             whose circumscribed disc lies inside the map marks at least one map cell.  The price is a dilation of at most half
 *             a map cell.  A translation by whole cells or a quarter turn with equal cell sizes puts all four samples into one
 *             frame cell: lossless.
 *   observation  of a map cell in a frame: OCCUPIED if any of the four samples reads exactly PWPP_OCC_OCCUPIED; otherwise FREE if
 *             all four read exactly PWPP_OCC_FREE; otherwise none.  Any other byte (a caller may have edited the image) counts as
 *             unknown.
 *   update    L is an int16_t per map cell, computed in int32.  OCCUPIED: L = min(L + hit, l_max).  FREE: L = max(L - miss,
 *             l_min).  None: unchanged.  The formulas apply as they stand to an input outside [l_min, l_max].
 *   order     map_of_frame[i] in [-1, n_maps) names frame i's map; -1: the frame is skipped; anything else: PWPP_E_ARG, naming
 *             the entry.  NULL with n_maps == 1: every frame updates map 0 -- a batch is a sequence.  NULL with n_maps == frames:
 *             frame i updates map i -- the lock-step streams.  NULL otherwise: PWPP_E_ARG.  A map's frames act in ASCENDING frame
 *             index; clamping makes the order matter: from L = 340 with hit 40, miss 20, l_max 350, a hit followed by a miss
 *             gives 330, a miss followed by a hit 350.
 *   shift     map_out[k][jy][jx] starts from map_in[k][jy + sy_k][jx + sx_k], or from 0 where that lies outside the map or map_in
 *             is NULL; the call's frames act on that start.  m describes the OUT map: a caller whose vehicle moved two cells east
 *             passes x0 + 2 * cell and sx = 2.  |sx| and |sy| may exceed the map.  A map no frame names comes out as its shifted
 *             input.  map_out == map_in is allowed iff every shift is {0, 0} (each cell is then read and written by one lane); any
 *             other overlap of the byte ranges of map_in, map_out and map_occupancy: PWPP_E_ARG.
 *   byte      map_occupancy = PWPP_OCC_OCCUPIED where L >= occupied_at; otherwise PWPP_OCC_FREE where L <= free_at; otherwise
 *             PWPP_OCC_UNKNOWN.
 *   composition  Two calls, the second reading the first's map_out with no shift, give exactly one call over the concatenated
 *             frames.  The same bytes for every call, mem, alignment and value of the option "fusion_path".
 *   fuse_obstacles   the per-frame bytes are exactly the occupancy image pwpp_visibility_obstacles(g, h_min, h_max, min_count,
 *             origin_xy, n_origins, max_range, frame_first, frames) gives, written for the caller where asked for and kept in the
 *             handle's cluster buffer otherwise (with its count and first images); the maps are exactly what pwpp_fuse_grid gives
 *             for them.  Entry i of pose and map_of_frame belongs to frame frame_first + i.  When, the grid's flags, the lifetime
 *             rule of the INPUT and the errors are those of pwpp_visibility_obstacles.
 *   mem       PWPP_MEM_HOST: every image and map is host memory, staged through the handle's cluster buffer; synchronous.
 *             PWPP_MEM_DEVICE: device memory -- maps 2-byte aligned, bytes byte aligned, no more -- enqueued on the handle's
 *             stream, complete after pwpp_synchronize.  PWPP_MEM_HOST_PINNED: PWPP_E_ARG.  pose, map_of_frame and shift are HOST
 *             memory always.
 *   errors    PWPP_E_ARG, named before the device is touched, in this order: a null handle, grid, occupancy (pwpp_fuse_grid),
 *             pose, map description or map_out; frames or a side of the frame image < 1, a side > 32768, nx * ny * frames beyond
 *             2^31; g->flags != 0 (pwpp_fuse_grid); the same three of n_maps and the map; a cell or CELL that is not finite and
 *             positive; hit, miss, the clamps and the thresholds outside the ranges at the struct; the number of poses;
 *             map_of_frame; the overlaps; mem.  pwpp_fuse_obstacles rejects first everything pwpp_visibility_obstacles rejects of
 *             its grid, band, min_count, max_range and origins, then the above of the map, and last the frame range and mem;
 *             before any estimate call: PWPP_E_STATE.
 *   buffers   No working image.  The poses, the frame lists (begin[n_maps + 1], frames[]) and the shifts are uploaded into the
 *             cluster buffer: allocated on first use, counted by pwpp_get_workspace_bytes, freed by pwpp_trim_workspace.
 *             pwpp_fuse_grid needs a handle for its stream and this buffer only.
 * With neither function called nothing is allocated or launched, and no result, state or timing of the estimate path changes. */
#define PWPP_HAS_OCCUPANCY_FUSION 1
typedef struct pwpp_fusion_map {     /* 56 bytes */
    double  x0, y0, cell;            /* the MAP's grid, in the fixed frame: cell (jx, jy) covers x0 + [jx, jx+1) * cell, ... */
    int32_t nx, ny;
    int32_t hit, miss;               /* added for an OCCUPIED / subtracted for a FREE observation; 0 .. 32767 */
    int32_t l_min, l_max;            /* clamps: -32768 <= l_min <= 0 <= l_max <= 32767 */
    int32_t occupied_at, free_at;    /* thresholds of the derived byte; -32768 <= free_at < occupied_at <= 32767 */
} pwpp_fusion_map;

/* any occupancy images: needs a handle (stream, buffer), no estimate call -- like pwpp_visibility_grid */
PWPP_API int pwpp_fuse_grid(pwpp_handle *h, const pwpp_ground_grid *g /* the FRAME images' grid; flags must be 0 */, int frames, int mem,
                            const int8_t *occupancy /* [frames][g->ny][g->nx] */,
                            const double *pose /* HOST, n_poses x 6 */, int n_poses,
                            const int32_t *map_of_frame /* HOST, frames entries, or NULL */,
                            const pwpp_fusion_map *m, int n_maps,
                            const int32_t *shift /* HOST, n_maps x {sx, sy} cells, or NULL: none */,
                            const int16_t *map_in /* [n_maps][m->ny][m->nx], or NULL: all zero */,
                            int16_t *map_out /* same shape */, int8_t *map_occupancy /* same shape, may be NULL */);
/* rasterize + visibility + fuse for frames of the LAST estimate call, one call -- like pwpp_visibility_obstacles */
PWPP_API int pwpp_fuse_obstacles(pwpp_handle *h, const pwpp_ground_grid *g, float h_min, float h_max, int min_count,
                                 const double *origin_xy, int n_origins, int max_range, int frame_first, int frames, int mem,
                                 const double *pose, int n_poses, const int32_t *map_of_frame,
                                 const pwpp_fusion_map *m, int n_maps, const int32_t *shift,
                                 const int16_t *map_in, int16_t *map_out, int8_t *map_occupancy /* may be NULL */,
                                 int8_t *occupancy /* the per-frame bytes, may be NULL: kept in the handle's buffer */);

/* ---- correlative scan match: where a frame's occupancy fits the fused map (pwpp_match_grid, pwpp_match_obstacles) ------------------
 * The fusion takes a pose per frame and trusts it; a map fused under a pose one cell or one degree off smears every wall.  The
 * match closes the chain: for a set of candidate poses and a window of whole-cell shifts it adds up the map's log-odds under the
 * frame's occupied cells and names the best (Olson 2009) -- integer sums, a total order for the maximum, so bit-reproducible.
 * estimate -> occupancy -> match -> fuse under the matched pose.  Below (X0, Y0, CELL, NX, NY) are m's fields (its update parameters
 * and thresholds are not read), (x0, y0, cell, nx, ny) g's.
 *   candidate A map-from-frame matrix {a, b, tx, c, d, ty}, exactly the fusion's pose; no angle enters the contract (the caller, or a
 *             binding's helper, builds the rotations).  HOST memory in both mem kinds, copied at the call: [n_sets][n_candidates][6],
 *             n_sets == 1: the same candidates for every frame; n_sets == frames: set i for frame i.  A candidate that is not
 *             finite is no error: its cells land nowhere.
 *   landing   For every cell (ix, iy) of frame f whose byte is exactly PWPP_OCC_OCCUPIED and every candidate r, all in double, every
 *             product, sum and quotient rounded on its own (no FMA, as in the fusion):
 *                 x = x0 + ((double)ix + 0.5) * cell          y alike
 *                 X = (a * x + b * y) + tx                    Y = (c * x + d * y) + ty
 *                 U = (X - X0) / CELL                         V alike
 *             The cell lands iff -1048576 <= U < 1048576 and the same for V (a NaN does not land); then Jx = (int)floor(U),
 *             Jy = (int)floor(V).
 *   score     For sx in [-wx, wx] and sy in [-wy, wy], scores[f][r][sy + wy][sx + wx] is the int64 sum of map[k][Jy + sy][Jx + sx]
 *             over the landed cells of (f, r); only cells with 0 <= Jx + sx < NX and 0 <= Jy + sy < NY contribute.  k is the frame's
 *             map by the fusion's map_of_frame rule: NULL with one map, NULL with one map per frame, or explicit.  A frame with
 *             map_of_frame == -1 is skipped: candidate -1, score 0, shift 0, cells still counted, its scores all 0.
 *   best      The maximum of the scores of a frame under this total order: the larger score; then the smaller sx * sx + sy * sy;
 *             then the smaller candidate index; then the smaller sy; then the smaller sx.  Callers put the prior first.  A frame
 *             with no occupied cell returns {0, 0, 0, 0, 0}.
 *   match_pose  Host only, no device needed: out is the candidate with tx + (double)sx * CELL and ty + (double)sy * CELL, one product
 *             and one sum each: what the caller hands to pwpp_fuse_* next.
 *   match_obstacles   the per-frame bytes are exactly the occupancy image pwpp_visibility_obstacles gives for the same arguments,
 *             written for the caller where asked for and kept in the handle's cluster buffer otherwise; best and scores are exactly
 *             what pwpp_match_grid gives for them.  Entry i of the candidate sets and of map_of_frame belongs to frame frame_first
 *             + i.  When, the lifetime rule of the INPUT and PWPP_E_STATE are those of pwpp_fuse_obstacles.
 *   mem       PWPP_MEM_HOST: images, map, best and scores are host memory, staged through the cluster buffer; synchronous.
 *             PWPP_MEM_DEVICE: device memory -- the map 2-byte aligned, the bytes byte aligned, no more; best and scores 8-byte
 *             aligned -- enqueued on the handle's stream, complete after pwpp_synchronize.  PWPP_MEM_HOST_PINNED: PWPP_E_ARG.
 *             candidates and map_of_frame are HOST memory always.
 *   errors    PWPP_E_ARG, named before the device is touched, in this order: a null handle, grid, occupancy (pwpp_match_grid),
 *             candidates, map description, map or best; frames or a side of the frame image < 1, a side > 32768, nx * ny * frames
 *             beyond 2^31; g->flags != 0 (pwpp_match_grid); the same three of n_maps and the map; a cell or CELL that is not finite
 *             and positive; n_candidates outside 1 .. 256; n_sets neither 1 nor frames; wx or wy outside 0 .. 64; frames *
 *             n_candidates beyond 2^24; with scores, their element count beyond 2^31; map_of_frame; mem; in PWPP_MEM_DEVICE a best
 *             or scores that is not 8-byte aligned.  pwpp_match_obstacles rejects first everything pwpp_visibility_obstacles
 *             rejects of its grid, band, min_count, max_range and origins, then the above of the map, and last the frame range and
 *             mem; before any estimate call: PWPP_E_STATE.
 *   buffers   The candidates and the frames' maps are uploaded into the cluster buffer; the frames' occupied cells (one packed word
 *             each, at most nx * ny per frame) and the workgroups' bests are working words there: allocated on first use, counted by
 *             pwpp_get_workspace_bytes, freed by pwpp_trim_workspace.
 *   outputs   The same bytes for every call, mem, alignment and value of the option "match_path".
 * With none of the three called nothing is allocated or launched, and no result, state or timing of any other call changes. */
#define PWPP_HAS_SCAN_MATCH 1
typedef struct pwpp_match_best {   /* 24 bytes, 8-byte aligned */
    int64_t score;                 /* the winning sum */
    int32_t candidate;             /* index into the frame's candidates; -1: the frame was skipped */
    int32_t sx, sy;                /* the winning shift, whole MAP cells */
    int32_t cells;                 /* occupied cells of the frame (bytes == PWPP_OCC_OCCUPIED) */
} pwpp_match_best;

/* any occupancy images and maps: needs a handle (stream, buffer), no estimate call -- like pwpp_fuse_grid */
PWPP_API int pwpp_match_grid(pwpp_handle *h, const pwpp_ground_grid *g /* the FRAME images' grid; flags must be 0 */, int frames, int mem,
                             const int8_t *occupancy /* [frames][g->ny][g->nx] */,
                             const double *candidates /* HOST, [n_sets][n_candidates][6] */, int n_sets /* 1 or frames */, int n_candidates,
                             const int32_t *map_of_frame /* HOST, frames entries, or NULL: the fusion's rule */,
                             const pwpp_fusion_map *m /* only x0, y0, cell, nx, ny are read */, int n_maps,
                             const int16_t *map /* [n_maps][m->ny][m->nx] */, int wx, int wy,
                             pwpp_match_best *best /* [frames] */,
                             int64_t *scores /* [frames][n_candidates][2 wy + 1][2 wx + 1], may be NULL */);
/* rasterize + visibility + match for frames of the LAST estimate call, one call -- like pwpp_fuse_obstacles */
PWPP_API int pwpp_match_obstacles(pwpp_handle *h, const pwpp_ground_grid *g, float h_min, float h_max, int min_count,
                                  const double *origin_xy, int n_origins, int max_range, int frame_first, int frames, int mem,
                                  const double *candidates, int n_sets, int n_candidates, const int32_t *map_of_frame,
                                  const pwpp_fusion_map *m, int n_maps, const int16_t *map, int wx, int wy,
                                  pwpp_match_best *best, int64_t *scores /* may be NULL */,
                                  int8_t *occupancy /* the per-frame bytes, may be NULL: kept in the handle's buffer */);
PWPP_API int pwpp_match_pose(const double candidate[6], double CELL, int sx, int sy, double out[6]);  /* host only */

/* ---- persistent elevation maps: per-frame ground heights fused over time (pwpp_fuse_height_grid, pwpp_fuse_ground) ----------------
 * The elevation image of a frame (pwpp_rasterize_ground) is NaN wherever the scan supports no ground model: bins with too few
 * points, shadowed sectors, everything beyond max_range.  A map a planner can drive on keeps the ground height under cells that
 * were seen three frames ago: the running mean of the heights observed per cell of a FIXED frame -- the ground half of the 2.5-D
 * map whose obstacle half pwpp_fuse_* keeps.  Integer state and a fixed arithmetic, so the fused map is a function of its inputs
 * alone and bit-reproducible.  The maps are the caller's arrays; a handle holds nothing of them between calls.  All n_maps maps
 * share the geometry and n_max of *m.  Below (X0, Y0, CELL, NX, NY) are m's fields, (x0, y0, cell, nx, ny) g's, M = 2^20.
 *   reused    pose, n_poses, map_of_frame, shift, mem, the composition of two calls and "HOST memory, copied at the call" are the
 *             occupancy fusion's (above), word for word: the pose is map-from-frame {a, b, tx, c, d, ty} and its inverse the
 *             TRANSPOSE; map_of_frame is NULL with one map, NULL with n_maps == frames, or explicit with -1: skipped; a map's
 *             frames act in ASCENDING frame index; a pose that is not finite observes nothing.
 *   z_offset  tz_f, the height of frame f's origin in the map's frame: HOST memory, n_poses doubles beside the poses (entry i with
 *             pose i), or NULL: 0.  A z_offset that is not finite is no error: its frame observes nothing.
 *   sample    ONE sample per map cell, at its centre.  Heights are a dense field: where a frame has a height under the centre it
 *             is the height there, so the four-quadrant argument of the occupancy fusion (a thin obstacle must not vanish) does
 *             not apply, and four samples would only blur steps.  All in double, every operation rounded on its own, no FMA:
 *                 mx = X0 + ((double)jx + 0.5) * CELL                          my alike with jy, Y0
 *                 dx = mx - tx;  dy = my - ty
 *                 fx = a * dx + c * dy;   fy = b * dx + d * dy
 *                 u = (fx - x0) / cell;  ix = (int)floor(u), inside iff 0 <= u && u < nx      v, iy alike with fy, y0, ny
 *             A sample outside the frame image, or whose u or v is a NaN, observes nothing.
 *   observation  Z = (double)height[f][iy][ix] + tz_f, one add.  The sample observes iff Z is finite and |Z| <= 1024.0; then
 *             q = llrint(Z * 1024), ties to even (the product is exact): units of 2^-10 m, |q| <= M.  A NaN height -- a cell the
 *             frame has no ground for -- observes nothing.
 *   state     A cell holds n, the observations it remembers (int16), and sum, the sum of their q (int32).  At the start of a call
 *             a cell's input is normalised: n = min(max(n_in, 0), n_max), then sum = min(max(sum_in, -n * M), n * M) in 64 bits:
 *             any caller data is legal.
 *   update    n < n_max: sum += q; n += 1 -- the exact running sum.  Otherwise: sum = sum - sum / n + q with C's integer division,
 *             truncating toward zero -- the mean forgets one share of itself.  |sum| <= n * M is an invariant (|s| - floor(|s| / n)
 *             <= (n - 1) * M), so with n_max <= 1023 an int32 never overflows.
 *   mean      mean = (float)(((double)sum / (double)n) / 1024.0): one division, one exact scaling, one rounding; the quiet NaN
 *             0x7fc00000 where n == 0.
 *   order     Below n_max the result does not depend on the order of a map's frames.  Once capped it does: with n_max 1, heights
 *             1.0 then 2.0 leave the mean 2.0, heights 2.0 then 1.0 leave 1.0; with n_max 2 from {n 2, sum 3072} (mean 1.5),
 *             q 1024 then 3072 gives 4352, q 3072 then 1024 gives 3328.
 *   shift     sum_out[k][jy][jx] and n_out[k][jy][jx] start from sum_in and n_in at [k][jy + sy_k][jx + sx_k], which read as 0
 *             outside the map or with both NULL (both NULL: empty maps; exactly one NULL: PWPP_E_ARG); m describes the OUT map.
 *             In place (sum_out == sum_in, n_out == n_in, either or both) is allowed iff every shift is {0, 0}; any other overlap
 *             of the byte ranges of sum_in, n_in, sum_out, n_out and mean: PWPP_E_ARG.
 *   composition  Two calls, the second reading the first's sum_out and n_out with no shift, give exactly one call over the
 *             concatenated frames.  The same bytes for every call, mem, alignment and value of the option "elevation_path".
 *   fuse_ground  the per-frame images are exactly what pwpp_rasterize_ground(g, frame_first, frames) gives, the NaN blanking of
 *             PWPP_GRID_GROUND_ONLY included, written for the caller where asked for and kept in the handle's cluster buffer
 *             otherwise; the maps are exactly what pwpp_fuse_height_grid gives for them.  Works after every kind of estimate call;
 *             before any: PWPP_E_STATE.  Entry i of pose, z_offset and map_of_frame belongs to frame frame_first + i.
 *   mem       PWPP_MEM_HOST: every image and map is host memory, staged through the handle's cluster buffer; synchronous.
 *             PWPP_MEM_DEVICE: device memory -- sum, mean and height 4-byte aligned, n 2-byte aligned, no more -- enqueued on the
 *             handle's stream, complete after pwpp_synchronize.  PWPP_MEM_HOST_PINNED: PWPP_E_ARG.  pose, z_offset, map_of_frame
 *             and shift are HOST memory always.
 *   errors    PWPP_E_ARG, named before the device is touched, in this order: a null handle, grid, height (pwpp_fuse_height_grid),
 *             pose, map description, sum_out or n_out; frames or a side of the frame image < 1, a side > 32768, nx * ny * frames
 *             beyond 2^31 (pwpp_fuse_height_grid; pwpp_fuse_ground names the product with the frame range); g->flags != 0
 *             (pwpp_fuse_height_grid) or other than 0 or PWPP_GRID_GROUND_ONLY (pwpp_fuse_ground); the same three of n_maps and the
 *             map; a cell or CELL that is not finite and positive; n_max outside 1 .. 1023; pad_ != 0; the number of poses;
 *             map_of_frame; exactly one of sum_in and n_in null; the overlaps; mem; in PWPP_MEM_DEVICE an array below its
 *             alignment.  pwpp_fuse_ground checks last what pwpp_rasterize_ground checks: the grid's origin, mem, PWPP_E_STATE
 *             before any estimate call, the frame range.
 *   buffers   No working image.  The poses, the offsets, the frame lists and the shifts are uploaded as one section of the cluster
 *             buffer: allocated on first use, counted by pwpp_get_workspace_bytes, freed by pwpp_trim_workspace.
 *             pwpp_fuse_height_grid needs a handle for its stream and this buffer only.
 * With neither function called nothing is allocated or launched, and no result, state or timing of any other call changes. */
#define PWPP_HAS_ELEVATION_FUSION 1
typedef struct pwpp_height_map {   /* 40 bytes */
    double  x0, y0, cell;          /* the MAP's grid in the fixed frame, as in pwpp_fusion_map */
    int32_t nx, ny;
    int32_t n_max;                 /* observations a cell's mean remembers: 1 .. 1023 */
    int32_t pad_;                  /* 0 */
} pwpp_height_map;

/* any height images: needs a handle (stream, buffer), no estimate call -- like pwpp_fuse_grid */
PWPP_API int pwpp_fuse_height_grid(pwpp_handle *h, const pwpp_ground_grid *g /* the FRAME images' grid; flags must be 0 */, int frames, int mem,
                                   const float *height /* [frames][g->ny][g->nx]; NaN: no height */,
                                   const double *pose /* HOST, n_poses x 6, the fusion's pose */,
                                   const double *z_offset /* HOST, n_poses, or NULL: 0 */, int n_poses,
                                   const int32_t *map_of_frame /* HOST, frames entries, or NULL */,
                                   const pwpp_height_map *m, int n_maps,
                                   const int32_t *shift /* HOST, n_maps x {sx, sy} cells, or NULL: none */,
                                   const int32_t *sum_in, const int16_t *n_in /* [n_maps][m->ny][m->nx]; both NULL: empty maps */,
                                   int32_t *sum_out, int16_t *n_out, float *mean /* same shape, may be NULL */);
/* rasterize_ground + fuse for frames of the LAST estimate call, one call -- like pwpp_fuse_obstacles */
PWPP_API int pwpp_fuse_ground(pwpp_handle *h, const pwpp_ground_grid *g /* flags: 0 or PWPP_GRID_GROUND_ONLY */,
                              int frame_first, int frames, int mem,
                              const double *pose, const double *z_offset, int n_poses, const int32_t *map_of_frame,
                              const pwpp_height_map *m, int n_maps, const int32_t *shift,
                              const int32_t *sum_in, const int16_t *n_in, int32_t *sum_out, int16_t *n_out, float *mean /* may be NULL */,
                              float *height /* the per-frame images, may be NULL: kept in the handle's buffer */);

/* ---- terrain analysis of height images: step, slope, roughness, traversability cost (pwpp_terrain_grid, pwpp_terrain_ground) ------
 * A height image says where the ground is, not whether a vehicle can stand or drive there.  For every cell these calls look at the
 * (2r+1) x (2r+1) window around it and give the height step inside it, the slope of the least-squares plane through it, the
 * roughness left after that plane is taken out, how many cells of the window are known, and a cost byte folded from the three.
 * `height` is any height image: a frame's elevation image (pwpp_rasterize_ground) or the fused `mean` of n_maps elevation maps
 * (pwpp_fuse_height_grid; then frames = n_maps).  The window sums are exact integers and the floating-point tail is written out
 * operation by operation, so every output is a function of the heights alone and bit-reproducible.  Below r = p->radius.
 *   known     A cell is known iff its height is finite and |height| <= 1024.0; then z = rint((double)height * 1024), ties to even
 *             (the product is exact): the elevation fusion's observation with tz = 0, units of 2^-10 m, |z| <= 2^20.  -0.0 is 0.
 *   window    of cell (ix, iy): the KNOWN cells (ix + dx, iy + dy), |dx|, |dy| <= r, that lie inside the frame's image; a cell
 *             outside the image is unknown (the window is clipped, never clamped or wrapped, and never reaches another frame).
 *             count = k, their number (<= 81), written for EVERY cell whether its centre is known or not.
 *   centre unknown   step, slope and rough are the quiet NaN 0x7fc00000, cost is -1.
 *   step      (float)((double)(zmax - zmin) / 1024.0) over the window: exact; 0 for k == 1.
 *   moments   As mathematical integers over the window with x = dx, y = dy: the sums Sx, Sy, Sz, Sxx, Sxy, Syy, Sxz, Syz, Szz;
 *             Cuv = k * Suv - Su * Sv;  D = Cxx * Cyy - Cxy^2;  A = Cxz * Cyy - Cyz * Cxy;  B = Cyz * Cxx - Cxz * Cxy;
 *             N = D * Czz - A * Cxz - B * Cyz.  The least-squares plane has the gradient (A / D, B / D) in height units per cell
 *             and the mean squared residual N / (D * k^2).  Adding one integer to every z changes none of D, A, B, N.
 *   degenerate  D == 0: fewer than three known cells, or all of them on one line.  Then slope and rough are the quiet NaN and cost
 *             is -1; step and count are defined all the same.
 *   bounds    (r <= 4; csrc/pwpp_terrain.h has the proofs) Cxx, Cyy <= 43740; 0 <= D < 2^31; Czz <= 81^2 * 2^40 < 2^53; |Cxz|,
 *             |Cyz| <= sqrt(Cxx * Czz) < 2^35; |A|, |B| < 2^51, exact in a double: all in int64.  0 <= N < 2^85 (Cauchy-Schwarz)
 *             needs 128 bits; Nd is its nearest double, ties to even.
 *   slope     In double, every operation rounded on its own, no FMA; rise over run:
 *                 slope = (float)(sqrt((double)A * (double)A + (double)B * (double)B) / ((double)D * (1024.0 * cell)))
 *   rough     rough = (float)(sqrt(Nd / ((double)D * (double)(k * k))) / 1024.0), metres.
 *   cost      a traversability byte in the value range of the visibility operator's nav_msgs/OccupancyGrid byte: -1 as stated
 *             above and where k < min_known; otherwise t = max(step / step_max, slope / slope_max, rough / rough_max), the ratios
 *             in double from the float outputs and the float limits, an infinite limit giving the ratio 0 (that test is off);
 *             cost = t >= 1 ? 100 : (int)floor(t * 100.0).
 *   outputs   An output that is NULL is not written; a call may ask for cost alone.  All five NULL: PWPP_E_ARG.
 *   overlaps  If any two of the caller's arrays overlap -- height against an output included -- PWPP_E_ARG.
 *   terrain_ground  the per-frame images are exactly what pwpp_rasterize_ground(g, frame_first, frames) gives, the NaN blanking of
 *             PWPP_GRID_GROUND_ONLY included, written for the caller where asked for and kept in the handle's cluster buffer
 *             otherwise; the outputs are exactly what pwpp_terrain_grid gives for them with cell = g->cell.  Works after every
 *             kind of estimate call; before any: PWPP_E_STATE.
 *   mem       PWPP_MEM_HOST: every image is host memory, staged through the handle's cluster buffer; synchronous.
 *             PWPP_MEM_DEVICE: device memory -- height, step, slope and rough 4-byte aligned, count and cost at any address --
 *             enqueued on the handle's stream, complete after pwpp_synchronize.  PWPP_MEM_HOST_PINNED: PWPP_E_ARG.
 *   errors    PWPP_E_ARG, named before the device is touched, in this order: a null handle, height (pwpp_terrain_grid) or grid
 *             (pwpp_terrain_ground), parameters; all five outputs null; frames or a side < 1, a side > 32768, nx * ny * frames
 *             beyond 2^31 (pwpp_terrain_grid; pwpp_terrain_ground names the product with the frame range); a cell that is not
 *             finite and positive (pwpp_terrain_grid) or g->flags other than 0 or PWPP_GRID_GROUND_ONLY (pwpp_terrain_ground);
 *             radius outside 1 .. 4; min_known outside 1 .. (2r+1)^2; a limit that is a NaN or not > 0; pad_ != 0; the overlaps;
 *             mem and, in PWPP_MEM_DEVICE, a float image below its alignment (pwpp_terrain_grid).  pwpp_terrain_ground checks last
 *             what pwpp_rasterize_ground checks -- the grid's origin and cell, mem, PWPP_E_STATE before any estimate call, the
 *             frame range -- and then the alignment.
 *   buffers   No working image and no upload: the parameters travel in the launch.  The cluster buffer holds the staged images
 *             (PWPP_MEM_HOST) and the kept raster; counted by pwpp_get_workspace_bytes, freed by pwpp_trim_workspace.
 *             pwpp_terrain_grid needs a handle for its stream and this buffer only.
 * The same bytes for every mem, alignment and value of the option "terrain_path".  With neither function called nothing is
 * allocated or launched, and no result, state or timing of any other call changes. */
#define PWPP_HAS_TERRAIN 1
typedef struct pwpp_terrain_params {   /* 24 bytes */
    int32_t radius;      /* r: the window is (2r+1) x (2r+1) cells; 1 .. 4 */
    int32_t min_known;   /* fewest known cells in the window for a cost; 1 .. (2r+1)^2 */
    float   step_max, slope_max, rough_max;  /* metres, rise over run, metres: each > 0, +inf allowed (that test is off), not NaN */
    int32_t pad_;        /* 0 */
} pwpp_terrain_params;

/* any height images: needs a handle (stream, buffer), no estimate call -- like pwpp_fuse_height_grid */
PWPP_API int pwpp_terrain_grid(pwpp_handle *h, int nx, int ny, int frames, double cell, int mem,
                               const float *height /* [frames][ny][nx]; NaN: unknown */, const pwpp_terrain_params *p,
                               float *step, float *slope, float *rough, uint8_t *count, int8_t *cost /* same shape; each may be NULL, not all */);
/* rasterize_ground + terrain for frames of the LAST estimate call, one enqueued sequence -- like pwpp_fuse_ground */
PWPP_API int pwpp_terrain_ground(pwpp_handle *h, const pwpp_ground_grid *g /* flags: 0 or PWPP_GRID_GROUND_ONLY */, int frame_first, int frames, int mem,
                                 const pwpp_terrain_params *p, float *step, float *slope, float *rough, uint8_t *count, int8_t *cost,
                                 float *height /* the per-frame images, may be NULL: kept in the handle's buffer */);

/* ---- cost to reach: exact shortest paths over a cost image from one source cell per frame (pwpp_reach_grid, pwpp_reach_ground) ----
 * The first thing a planner asks of a cost image: what does it cost to get from where the vehicle stands to every cell, and through
 * which neighbour.  For every frame these calls give that field over the 8-connected cells in integers.  With positive integer
 * step costs the field is the one fixed point of the relaxation, so every schedule of the kernels gives the same bytes as a
 * Dijkstra on the host; no floating point is involved.  Each frame is on its own; frames never influence each other.
 *   cost      cost[f][iy][ix], an int8 in the value range of the terrain operator's `cost` and the visibility operator's
 *             `occupancy`: c < 0 unknown, 0 .. 100 a traversal cost, anything >= lethal impassable.
 *   params    base 1 .. 255, what a cell of free ground costs; lethal 1 .. 101 (101: no value is lethal); unknown -1 .. 100 (-1: an
 *             unknown cell is impassable; otherwise it counts as that cost byte, and the lethal rule applies to it as to any
 *             cost); clearance2 >= 0, read only when dist2 != NULL; max_reach >= 0 (0: unlimited); pad_ 0.
 *   passable  A cell is passable iff its (possibly substituted) cost is in 0 .. lethal - 1 and (dist2 == NULL or dist2[cell] >
 *             clearance2).  dist2 is the image of pwpp_distance_grid (squared cells, PWPP_DIST_BEYOND allowed); with it,
 *             clearance2 = 0 blocks the occupied cells themselves.  The source cell is passable whatever its bytes say -- it holds
 *             the vehicle -- as the visibility operator's origin never blocks.
 *   term      t(cell) = base + cost for a passable cell; t = base for a source that is passable only by the rule above.  t <= base + 100.
 *   step      from a to one of its 8 neighbours b, both passable and inside the image: step(a, b) = w * (t(a) + t(b)), w = 5 across
 *             an edge and w = 7 across a corner.  A corner step exists only if both cells that share an edge with a and with b are
 *             passable: paths do not cut corners and do not squeeze between two diagonal blocked cells, the stance of the
 *             visibility walk.  step is symmetric, so the field from a goal equals the field to it.  The weights 5 and 7 are the
 *             contract, not an approximation of anything.
 *   reach     reach[f][iy][ix], an int32: the minimum over all step paths from the frame's source of the sum of steps; 0 at the
 *             source; PWPP_REACH_NONE where no path exists.
 *   from      from[f][iy][ix], an int32, may be NULL: among the neighbours n with an existing step n -> c and reach[n] + step(n, c)
 *             == reach[c], the smallest index jy * nx + jx.  The source's own index at the source; -1 where reach is
 *             PWPP_REACH_NONE.  A function of the reach image and the passability alone.  Following from ends at the source,
 *             because reach strictly decreases along it.
 *   max_reach > 0: every cell whose true value exceeds it reports PWPP_REACH_NONE / -1, and every other cell exactly what the
 *             unlimited call gives (every prefix of a shortest path is no dearer than the path): it bounds the work and is not an
 *             approximation.
 *   range     14 * (base + 100) * (nx * ny - 1) <= 2^31 - 2, evaluated in 64 bits; otherwise PWPP_E_ARG, naming the product.  It
 *             keeps every true value below PWPP_REACH_NONE in 32 bits (csrc/pwpp_reach.h has the proof).
 *   sources   one cell per frame, given as the visibility's origins are: n_sources is 1 (for every frame) or `frames`.
 *             pwpp_reach_grid: n_sources x {sx, sy}, host memory whatever `mem`, copied at the call.  pwpp_reach_ground: metres,
 *             turned into cells by the raster's cell rule.  A source outside the image, a position that is not finite, any other
 *             count: PWPP_E_ARG, naming the entry.
 *   reach_ground  enqueues pwpp_rasterize_ground(g, frame_first, frames), pwpp_terrain_grid for its cost alone and the reach, as
 *             one sequence.  The cost image is exactly what pwpp_terrain_ground gives, written for the caller where asked for and
 *             kept in the handle's cluster buffer otherwise.  No dist2 in this call.  Before any estimate call: PWPP_E_STATE.
 *   mem       PWPP_MEM_HOST: every image is host memory, staged through the handle's cluster buffer; synchronous.
 *             PWPP_MEM_DEVICE: device memory -- dist2, reach and from 4-byte aligned, the cost bytes at any address -- enqueued on
 *             the handle's stream, complete after pwpp_synchronize.  PWPP_MEM_HOST_PINNED: PWPP_E_ARG.
 *   errors    PWPP_E_ARG, named before the device is touched, in this order.  pwpp_reach_grid: a null handle, cost, parameters,
 *             source, reach; frames or a side < 1, a side > 32768, nx * ny * frames beyond 2^31; base, lethal, unknown, clearance2
 *             (with dist2 only), max_reach, pad_; the range; the count of sources, then the first source outside the image; two of
 *             the caller's images overlapping; mem; in PWPP_MEM_DEVICE an int32 image below its alignment.  pwpp_reach_ground: a
 *             null handle, grid, terrain parameters, reach parameters, source, reach; frames or a side < 1, a side > 32768,
 *             g->flags other than 0 or PWPP_GRID_GROUND_ONLY; the terrain parameters as pwpp_terrain_ground names them; the reach
 *             parameters and the range as above; the grid's origin and cell; the count of sources, then the first that is not
 *             finite or lies outside the grid; the overlaps; then what pwpp_rasterize_ground checks -- mem, PWPP_E_STATE before
 *             any estimate call, the frame range, the product beyond 2^31 -- and the alignment.
 *   defect    Every loop of the kernels has a bound derived from the image (at most nx * ny + 1 sweeps over the image or passes over
 *             its tiles, at most tile cells + 1 sweeps per visit of a tile).  By the fixed-point argument only a defect of the
 *             library can reach it; then no kernel loops on: PWPP_MEM_HOST returns PWPP_E_HIP, "internal error", and in
 *             PWPP_MEM_DEVICE reach is PWPP_REACH_NONE at the source of such a frame, which no result has.  The from pass does not
 *             write the field: a value it finds no predecessor for (a defect too) is reported the same way in PWPP_MEM_HOST and
 *             shows in PWPP_MEM_DEVICE as from = -1 beside a reach that is not PWPP_REACH_NONE, which no result has either.
 *   buffers   Working memory -- a uint16 per cell, one word, the uploaded sources -- and in PWPP_MEM_HOST the staged images lie in the
 *             cluster buffer; counted by pwpp_get_workspace_bytes, freed by pwpp_trim_workspace.  pwpp_reach_grid needs a handle for
 *             its stream and this buffer only.
 * The same bytes for every mem, alignment and value of the option "reach_path".  With neither function called nothing is
 * allocated or launched, and no result, state or timing of any other call changes. */
#define PWPP_HAS_REACH 1
#define PWPP_REACH_NONE 0x7fffffff
typedef struct pwpp_reach_params {   /* 24 bytes */
    int32_t base;        /* what a cell of free ground costs; 1 .. 255 */
    int32_t lethal;      /* a cost byte >= lethal is impassable; 1 .. 101 (101: none is) */
    int32_t unknown;     /* -1: an unknown cell (cost < 0) is impassable; 0 .. 100: it counts as this cost byte */
    int32_t clearance2;  /* with dist2: passable needs dist2 > clearance2 (squared cells); >= 0 */
    int32_t max_reach;   /* 0: unlimited; > 0: cells beyond it report PWPP_REACH_NONE */
    int32_t pad_;        /* 0 */
} pwpp_reach_params;

/* any cost images: needs a handle (stream, buffer), no estimate call -- like pwpp_terrain_grid */
PWPP_API int pwpp_reach_grid(pwpp_handle *h, int nx, int ny, int frames, int mem, const int8_t *cost /* [frames][ny][nx] */,
                             const int32_t *dist2 /* same shape, may be NULL */, const pwpp_reach_params *p,
                             const int32_t *source /* host: n_sources x {sx, sy} */, int n_sources /* 1 or frames */,
                             int32_t *reach /* same shape */, int32_t *from /* same shape, may be NULL */);
/* rasterize_ground + the terrain's cost + reach for frames of the LAST estimate call, one enqueued sequence -- like pwpp_terrain_ground */
PWPP_API int pwpp_reach_ground(pwpp_handle *h, const pwpp_ground_grid *g /* flags: 0 or PWPP_GRID_GROUND_ONLY */, int frame_first, int frames, int mem,
                               const pwpp_terrain_params *terrain_params, const pwpp_reach_params *reach_params,
                               const double *source_xy /* host: n_sources x {x, y}, metres */, int n_sources, int32_t *reach, int32_t *from /* may be NULL */,
                               int8_t *cost /* the terrain's cost bytes, may be NULL: kept in the handle's buffer */);
/* The raster's cell rule for one position in metres, as pwpp_reach_ground applies it to a source and pwpp_visibility_obstacles to an
 * origin: cell (ix, iy) of the grid's origin, cell size and sides (flags are not read), for a caller of pwpp_reach_grid who has metres.
 * PWPP_E_ARG, named: a null grid or result, a grid without cells or with an origin or cell size that is not finite and positive, a
 * position that is not finite, a position outside the grid.  Needs no handle and touches no device. */
PWPP_API int pwpp_grid_cell_of(const pwpp_ground_grid *g, double x, double y, int32_t *ix, int32_t *iy);

/* ---- cluster tracks: which cluster of this frame is which cluster of the frame before (pwpp_associate_grid, pwpp_track_obstacles) ----
 * The labels of pwpp_label_grid are per frame: row 3 of one frame and row 3 of the next have nothing to do with each other.  These
 * calls relate the two label images of one stream: how many cells every pair of rows shares, each row's best partner on both
 * sides, and optionally an id that a cluster keeps from frame to frame.  Everything is an integer count or an argmax under a
 * total order: a function of the inputs alone, the same bytes for every mem, alignment and schedule of the kernels.  Each frame
 * pair is on its own.
 *   inputs    per frame pair f: prev[f], an int32 label image on the grid gp; curr[f], one on the grid gc; a pose {a, b, tx, c, d, ty}
 *             that says where a position of the previous frame lies in the current frame -- exactly the meaning of the fusion's
 *             map-from-frame pose (pwpp_fuse_grid), with the current grid in the role of the map and the previous image in the role
 *             of the frame.  n_poses is 1 (for every frame) or `frames`; poses are host memory whatever `mem`, copied at the call.
 *             gc and gp are pwpp_ground_grid structures (origin, cell, sides) whose flags must be 0.  The images are as
 *             pwpp_label_grid writes them or edited by the caller.
 *   rows      A label l names a row iff 0 <= l < max_rows.  Every other value counts as unlabelled, on both sides, as
 *             pwpp_box_obstacles skips it.
 *   previous cell  of a current cell (jx, jy): its centre by the elevation fusion's rule, x = gc.x0 + ((double)jx + 0.5) * gc.cell,
 *             carried into gp by the fusion's sample rule (the transpose as the inverse, in double, every operation rounded on its own,
 *             the cell rule of the obstacle raster; the product with the exact reciprocal where the cell size is a power of two gives the same
 *             bits).  Where that position lies outside the previous image, is a NaN, or the pose is not finite, the cell has no
 *             previous cell and casts no vote, whatever the gate.
 *   vote      A current cell c with row b and previous cell p = (px, py) votes for one previous row: the row of the labelled
 *             previous cell d = (px + ex, py + ey) with |ex|, |ey| <= gate inside the previous image; among such cells the
 *             smallest ex^2 + ey^2 wins, then the smallest index (py + ey) * nxp + (px + ex).  No such cell: no vote.  gate is 0 .. 4;
 *             with gate 0 this is plain overlap.
 *   overlap   n(a, b) is the number of current cells of row b that vote for a.  A pair (a, b) exists iff n(a, b) > 0.
 *   links     curr_links[f][b]: cells = all current cells labelled b; links = the number of distinct a with n(a, b) > 0; other =
 *             the a with the largest n(a, b), the smallest a on a tie, -1 when links == 0; overlap = n(other, b), or 0.
 *             prev_links[f][a]: cells = all previous cells labelled a, whatever the pose; links = the number of distinct b with
 *             n(a, b) > 0; other = the b with the largest n(a, b), the smallest b on a tie, -1 without one; overlap likewise.
 *             links > 1 is a merge on the current side and a split on the previous side.  Both tables have max_rows rows per frame.
 *   pairs     n_pairs[f] (may be NULL) is the frame's number of distinct pairs when that is at most max_pairs.  Otherwise it is
 *             max_pairs + 1, and every row of both tables of that frame has other = -2, overlap = 0, links = 0, with cells still
 *             exact.  Overflow is a function of the inputs alone, never of the schedule: the pairs are counted in a table of
 *             2 * max_pairs slots per frame, and a table with at least 2 * max_pairs slots cannot fill before the count of
 *             distinct insertions passes max_pairs.
 *   ids       Optional: computed iff id_prev, next_id, id_curr and next_id_out are all non-null; some of them only: PWPP_E_ARG.
 *             id_prev[f][a] and id_curr[f][b] have max_rows entries per frame, next_id[f] and next_id_out[f] one.  A current row
 *             exists iff cells > 0.  An existing row b continues a iff curr_links[b].other == a with a >= 0, prev_links[a].other
 *             == b, overlap >= min_overlap and id_prev[f][a] >= 0; then id_curr[f][b] = id_prev[f][a].  Every other existing row is
 *             fresh: its id is (next_id[f] + k) & 0x7fffffff, k the number of fresh rows below b, in unsigned 32-bit arithmetic.
 *             Rows that do not exist get -1.  next_id_out[f] = (next_id[f] + the frame's fresh rows) & 0x7fffffff.  A mutual best
 *             is unique, so the ids of a frame stay distinct if those of id_prev were and lie below next_id (until the counter
 *             wraps).  An overflowed frame makes every existing row fresh, by the same rule.  min_overlap >= 1 is read with or without ids.
 *   track_obstacles  for frames of the LAST estimate call: enqueues pwpp_label_obstacles(g, h_min, h_max, min_count, connectivity,
 *             frame_first, frames, ...) and the association of that label image against the caller's prev_label on the same grid
 *             g (gc = gp = g with flags 0), max_rows = max_clusters, as one sequence.  label, count, top, clusters, n_clusters and
 *             point_cluster are exactly what pwpp_label_obstacles gives; the links and ids exactly what pwpp_associate_grid gives
 *             for those images.  Before any estimate call: PWPP_E_STATE.
 *   state     The handle keeps nothing between calls: the previous label image, the ids and next_id are the caller's, as the maps
 *             of the fusions are.  Feed label, id_curr and next_id_out of one step back as prev, id_prev and next_id of the next.
 *   mem       PWPP_MEM_HOST: every array but the poses is host memory, staged through the handle's cluster buffer; synchronous.
 *             PWPP_MEM_DEVICE: device memory, every array 4-byte aligned, enqueued on the handle's stream, complete after
 *             pwpp_synchronize.  PWPP_MEM_HOST_PINNED: PWPP_E_ARG.
 *   errors    PWPP_E_ARG, named before the device is touched, in this order.  pwpp_associate_grid: a null handle, current grid,
 *             previous grid, current image, previous image, pose, curr_links, prev_links; for gc and then for gp: frames or a side
 *             < 1, a side > 32768, nx * ny * frames beyond 2^31; the flags of gc, then of gp; origin and cell size of gc, then of gp;
 *             gate; min_overlap; max_rows < 1, then frames * max_rows > 2^24; max_pairs < 1, then frames * max_pairs > 2^24; the
 *             count of poses; the partial id set; two of the caller's arrays overlapping; mem; in PWPP_MEM_DEVICE an array below its
 *             alignment.  pwpp_track_obstacles: a null handle, grid, label image, previous label image, pose, curr_links,
 *             prev_links; then everything pwpp_label_obstacles rejects, in its order -- PWPP_E_STATE before any estimate call among
 *             it; then a side > 32768, grid flags other than 0, and the above from the gate on.
 *   buffers   Working memory -- the pair tables (12 bytes a slot), two 64-bit words per row, the uploaded poses -- and in
 *             PWPP_MEM_HOST the staged arrays lie in the cluster buffer; counted by pwpp_get_workspace_bytes, freed by
 *             pwpp_trim_workspace.  pwpp_associate_grid needs a handle for its stream and this buffer only, like pwpp_label_grid.
 * With neither function called nothing is allocated or launched, and no result, state or timing of any other call changes.
 * Not built: motion models and filtering, an assignment beyond the mutual best, track ages and deletion, velocities as an output
 * (INTEGRATION.md says how they follow from pwpp_box_obstacles), association across more than two frames, a list of the pairs. */
#define PWPP_HAS_CLUSTER_TRACKS 1
typedef struct pwpp_cluster_link {   /* 16 bytes */
    int32_t other;       /* the best partner row on the other side; -1: none; -2: the frame has more than max_pairs pairs */
    int32_t overlap;     /* n(other, this row), or 0 */
    int32_t cells;       /* all cells of this side's image labelled with this row */
    int32_t links;       /* the number of partner rows with n > 0 */
} pwpp_cluster_link;

/* any label images: needs a handle (stream, buffer), no estimate call -- like pwpp_label_grid */
PWPP_API int pwpp_associate_grid(pwpp_handle *h, const pwpp_ground_grid *gc, const pwpp_ground_grid *gp, int frames, int mem,
                                 const int32_t *curr /* [frames][gc.ny][gc.nx] */, const int32_t *prev /* [frames][gp.ny][gp.nx] */,
                                 const double *pose /* host: n_poses x {a, b, tx, c, d, ty} */, int n_poses /* 1 or frames */,
                                 int gate /* 0 .. 4 */, int min_overlap /* >= 1 */, int max_rows, int max_pairs,
                                 pwpp_cluster_link *curr_links, pwpp_cluster_link *prev_links /* [frames][max_rows] each */,
                                 int32_t *n_pairs /* [frames], may be NULL */,
                                 const int32_t *id_prev /* [frames][max_rows] */, const int32_t *next_id /* [frames] */,
                                 int32_t *id_curr /* [frames][max_rows] */, int32_t *next_id_out /* [frames]; all four or none */);
/* label_obstacles + the association against the caller's previous label image for frames of the LAST estimate call, one enqueued
 * sequence -- like pwpp_reach_ground.  The arguments up to point_cluster are pwpp_label_obstacles'. */
PWPP_API int pwpp_track_obstacles(pwpp_handle *h, const pwpp_ground_grid *g /* flags: 0 */, float h_min, float h_max, int min_count, int connectivity,
                                  int frame_first, int frames, int mem, int32_t *label, int32_t *count, float *top,
                                  pwpp_obstacle_cluster *clusters, int32_t *n_clusters, int max_clusters, int32_t *point_cluster,
                                  const int32_t *prev_label /* [frames][ny][nx] */, const double *pose, int n_poses, int gate, int min_overlap,
                                  int max_pairs, pwpp_cluster_link *curr_links, pwpp_cluster_link *prev_links /* [frames][max_clusters] each */,
                                  int32_t *n_pairs, const int32_t *id_prev, const int32_t *next_id, int32_t *id_curr, int32_t *next_id_out);

/* ---- map evidence: what the fused map holds under every cluster of a frame (pwpp_evidence_grid, pwpp_evidence_obstacles) -----------
 * Perception gives a label image per frame, the fusion a persistent log-odds map; these calls relate the two.  Every labelled cell of
 * a frame is carried into the map by the frame's pose and reads the map there; per cluster row the readings are counted by class
 * and a verdict says whether the cluster is part of the world the map already knows (static) or stands where the map has seen free
 * space (moving).  The masked occupancy bytes leave the movers out of the next fusion.  Integer counts and a verdict from integer
 * ratios: a total function of the inputs, the same bytes for every mem, alignment, schedule and value of the option "evidence_path".
 * estimate -> match -> visibility -> label -> evidence -> fuse the masked bytes.  Below (X0, Y0, CELL, NX, NY) are m's fields,
 * (x0, y0, cell, nx, ny) g's.
 *   inputs    per frame f: label[f], an int32 label image on the grid g (flags 0), as pwpp_label_grid writes it or edited by the
 *             caller; a map-from-frame pose {a, b, tx, c, d, ty}, exactly the fusion's pose and the match's candidate; the frame's
 *             map k by the fusion's map_of_frame rule (NULL with one map, NULL with one map per frame, or explicit; -1 skips the
 *             frame); int16 log-odds maps map[n_maps][NY][NX] described by m, of which x0, y0, cell, nx, ny, occupied_at and free_at
 *             are read.  n_poses is 1 (for every frame) or `frames`.  Poses and map_of_frame are HOST memory whatever mem, copied at
 *             the call.
 *   rows      A label l names a row iff 0 <= l < max_rows, as in pwpp_associate_grid.  Every other value is unlabelled.
 *   landing   A labelled cell (ix, iy) lands at (Jx, Jy) by the scan match's landing (pwpp_match_grid above: the cell's centre, the
 *             pose, the quotient by CELL, |U|, |V| < 1048576, the floor; no FMA) under the frame's pose.  The cell is LANDED iff it
 *             lands there and 0 <= Jx < NX and 0 <= Jy < NY.  A pose that is not finite lands nothing; a skipped frame lands nothing.
 *   reading   For a landed cell, E is the maximum of map[k][Jy + ey][Jx + ex] over |ex|, |ey| <= gate inside the map; gate is
 *             0 .. 4, with gate 0 E is the one cell.  The maximum is chosen so that a wall displaced by a pose error of up to `gate`
 *             cells still finds its wall -- the half-cell dilation of the fusion's four samples is a displacement of that kind --
 *             while a mover in swept free space finds only free cells.  THE PRICE: a mover within `gate` cells of a mapped wall
 *             reads as wall.
 *   class     of a landed cell, the fusion's byte rule applied to E: PWPP_OCC_OCCUPIED where E >= occupied_at; otherwise
 *             PWPP_OCC_FREE where E <= free_at; otherwise PWPP_OCC_UNKNOWN.
 *   row       rows[f][r]: cells = all cells labelled r; landed = those that landed; occupied, free and unknown count the landed
 *             cells by class (their sum is landed); sum = the int64 sum of E over the landed cells.  max_rows rows per frame.
 *   verdict   from rule = {gate, min_cells, moving_share, static_share}, min_cells >= 1, the shares 1 .. 256 in 256ths, evaluated
 *             in int64 in this order: PWPP_EVID_NONE where cells == 0; otherwise PWPP_EVID_MOVING where landed >= min_cells and
 *             free * 256 >= moving_share * landed; otherwise PWPP_EVID_STATIC where landed >= min_cells and occupied * 256 >=
 *             static_share * landed; otherwise PWPP_EVID_UNDECIDED.  pwpp_evidence_verdict is the same function on the host.
 *   cell_class  Optional, int8 [frames][ny][nx]: the class byte of a labelled, landed cell, PWPP_EVID_CELL_NONE for every other cell.
 *   occupancy_out  Optional, int8, together with occupancy_in: both or neither.  PWPP_OCC_UNKNOWN where the cell's label names a row
 *             whose verdict is PWPP_EVID_MOVING; everywhere else the input byte verbatim, whatever its value.  These are the bytes
 *             to hand to pwpp_fuse_grid so that the mover is not observed at all.  occupancy_out == occupancy_in, the same pointer,
 *             is allowed: each byte is read and written by one lane.  Any other overlap among the caller's arrays is an error.
 *   evidence_obstacles  for frames of the LAST estimate call: enqueues pwpp_label_obstacles(g, h_min, h_max, min_count, connectivity,
 *             frame_first, frames, ...) and the evidence of that label image with max_rows = max_clusters as one sequence.  label,
 *             count, top, clusters, n_clusters and point_cluster are exactly what pwpp_label_obstacles gives; rows, cell_class and
 *             occupancy_out exactly what pwpp_evidence_grid gives for that image.  Entry i of pose and map_of_frame belongs to frame
 *             frame_first + i.  Before any estimate call: PWPP_E_STATE.
 *   state     The handle keeps nothing between calls.  A verdict joins an id of pwpp_track_obstacles by its row: both use the row
 *             numbers of the same label image.
 *   mem       PWPP_MEM_HOST: every array but the poses and map_of_frame is host memory, staged through the handle's cluster buffer;
 *             synchronous.  PWPP_MEM_DEVICE: device memory -- rows 8-byte aligned, label 4, map 2, the byte images 1 -- enqueued on
 *             the handle's stream, complete after pwpp_synchronize.  PWPP_MEM_HOST_PINNED: PWPP_E_ARG.
 *   errors    PWPP_E_ARG, named before the device is touched, in this order.  pwpp_evidence_grid: a null handle, grid, label image,
 *             pose, map description, map, rule, rows; frames or a side of g < 1, a side > 32768, nx * ny * frames beyond 2^31; the
 *             same three of n_maps and the map; g->flags != 0; an origin or cell of g that is not finite, the cell positive; the
 *             same of the map; free_at < -32768, free_at >= occupied_at or occupied_at > 32767; gate outside 0 .. 4; min_cells < 1;
 *             moving_share, then static_share outside 1 .. 256; max_rows < 1, then frames * max_rows > 2^24; the count of poses;
 *             map_of_frame; one of occupancy_in and occupancy_out without the other; two of the caller's arrays overlapping; mem; in
 *             PWPP_MEM_DEVICE an array below its alignment.  pwpp_evidence_obstacles: a null handle, grid, label image, pose, map
 *             description, map, rule, rows; then everything pwpp_label_obstacles rejects, in its order -- PWPP_E_STATE before any
 *             estimate call among it; then a side > 32768, grid flags other than 0, and the above from the map's sizes on.
 *   buffers   The poses and the frames' maps are uploaded into the cluster buffer, where in PWPP_MEM_HOST the staged arrays lie
 *             too; counted by pwpp_get_workspace_bytes, freed by pwpp_trim_workspace.  The rows themselves take the kernels' sums:
 *             there are no working words.  pwpp_evidence_grid needs a handle for its stream and this buffer only, like
 *             pwpp_associate_grid.
 *   option    "evidence_path": 0 = the path the measurement chose, 1 = the sums go to the rows with global
 *             atomics, 2 = a workgroup sums a run of cells in LDS first, where max_rows <= PWPP_EVID_LDS_ROWS: 24 bytes a row, 12
 *             KiB, so that the tables of the eight workgroups of 256 lanes that make 8 waves a SIMD take 96 of a CU's 160 KiB;
 *             beyond that path 2 is path 1.
 * With neither function called nothing is allocated or launched, and no result, state or timing of any other call changes.
 * Not built: motion models, verdicts smoothed over time (the id of pwpp_track_obstacles lets a caller do that), free-space evidence
 * inside the match's score, erasing a trail that is already in the map. */
#define PWPP_HAS_MAP_EVIDENCE 1
#define PWPP_EVID_LDS_ROWS 512
enum { PWPP_EVID_NONE = -1, PWPP_EVID_UNDECIDED = 0, PWPP_EVID_STATIC = 1, PWPP_EVID_MOVING = 2 };   /* the verdict of a row */
enum { PWPP_EVID_CELL_NONE = -2 };   /* cell_class of a cell that is not labelled or not landed */
typedef struct pwpp_cluster_evidence {   /* 32 bytes, 8-byte aligned */
    int64_t sum;         /* the sum of E over the landed cells */
    int32_t cells;       /* all cells of the image labelled with this row */
    int32_t landed;      /* those that landed inside the map */
    int32_t occupied;    /* landed cells by class: E >= occupied_at */
    int32_t free;        /* ... E <= free_at */
    int32_t unknown;     /* ... between the two */
    int32_t verdict;     /* PWPP_EVID_* */
} pwpp_cluster_evidence;
typedef struct pwpp_evidence_rule {      /* 16 bytes */
    int32_t gate;          /* 0 .. 4 map cells */
    int32_t min_cells;     /* >= 1: fewer landed cells leave a row undecided */
    int32_t moving_share;  /* 1 .. 256, in 256ths of the landed cells */
    int32_t static_share;  /* 1 .. 256 */
} pwpp_evidence_rule;

/* any label images and maps: needs a handle (stream, buffer), no estimate call -- like pwpp_associate_grid */
PWPP_API int pwpp_evidence_grid(pwpp_handle *h, const pwpp_ground_grid *g /* the label images' grid; flags must be 0 */, int frames, int mem,
                                const int32_t *label /* [frames][g->ny][g->nx] */,
                                const int8_t *occupancy_in /* [frames][g->ny][g->nx], or NULL with occupancy_out NULL */,
                                const double *pose /* HOST: n_poses x {a, b, tx, c, d, ty} */, int n_poses /* 1 or frames */,
                                const int32_t *map_of_frame /* HOST, frames entries, or NULL: the fusion's rule */,
                                const pwpp_fusion_map *m, int n_maps, const int16_t *map /* [n_maps][m->ny][m->nx] */,
                                const pwpp_evidence_rule *rule, int max_rows,
                                pwpp_cluster_evidence *rows /* [frames][max_rows] */,
                                int8_t *cell_class /* [frames][g->ny][g->nx], may be NULL */,
                                int8_t *occupancy_out /* like occupancy_in, may be that pointer */);
/* label_obstacles + the evidence of its label image for frames of the LAST estimate call, one enqueued sequence -- like
 * pwpp_track_obstacles.  The arguments up to point_cluster are pwpp_label_obstacles'. */
PWPP_API int pwpp_evidence_obstacles(pwpp_handle *h, const pwpp_ground_grid *g /* flags: 0 */, float h_min, float h_max, int min_count, int connectivity,
                                     int frame_first, int frames, int mem, int32_t *label, int32_t *count, float *top,
                                     pwpp_obstacle_cluster *clusters, int32_t *n_clusters, int max_clusters, int32_t *point_cluster,
                                     const int8_t *occupancy_in, const double *pose, int n_poses, const int32_t *map_of_frame,
                                     const pwpp_fusion_map *m, int n_maps, const int16_t *map, const pwpp_evidence_rule *rule,
                                     pwpp_cluster_evidence *rows /* [frames][max_clusters] */, int8_t *cell_class, int8_t *occupancy_out);
/* host only, no device needed: *verdict = PWPP_EVID_* of a row with these counts (PWPP_EVID_NONE is -1, so the verdict is no return
 * value); PWPP_E_ARG for a null rule or verdict, a rule out of range, or counts that no row has (negative, landed > cells,
 * occupied + free > landed) */
PWPP_API int pwpp_evidence_verdict(const pwpp_evidence_rule *rule, int32_t cells, int32_t landed, int32_t occupied, int32_t free_cells,
                                   int32_t *verdict);

/* ---- costmap: occupancy, inflated obstacle distance and terrain cost folded into one cost byte (pwpp_costmap_grid, pwpp_costmap_obstacles) ----
 * The layers of a navigation costmap exist as separate images in separate value ranges: the visibility's (or the fusion's) occupancy
 * byte, the exact dist2 to the nearest obstacle, the terrain's traversability cost.  These calls join them into the one int8 cost
 * image pwpp_reach_grid takes.  The graded cost near an obstacle -- the inflation -- is DATA, not arithmetic: a table of bytes
 * indexed by the integer dist2, supplied by the caller (pwpp_costmap_curve builds a common one on the host).  The device gathers
 * and folds integers, so the costmap is a function of its inputs alone and bit-reproducible.  Cells and frames never influence
 * each other.
 *   params    layers: a bit mask, not 0, of PWPP_COSTMAP_OCCUPANCY (1), PWPP_COSTMAP_INFLATION (2), PWPP_COSTMAP_TERRAIN (4);
 *             occupancy_unknown and terrain_unknown -1 .. 100; unknown_below 1 .. 101; pad_ 0.
 *   curve     uint8 curve[n_curve], host memory whatever `mem`, copied at the call; 1 <= n_curve <= PWPP_COSTMAP_MAX_CURVE (4097:
 *             dist2 up to 64^2, a radius of 64 cells); every entry 0 .. 100.  Read only with PWPP_COSTMAP_INFLATION: without it
 *             curve may be NULL and n_curve 0, and neither is looked at.
 *   inputs    per cell o (the occupancy byte), t (the terrain byte) and d (dist2), each read only when its layer is enabled.
 *   occupancy o == PWPP_OCC_OCCUPIED gives 100; o == PWPP_OCC_FREE gives 0; any other byte is unknown, as the fusion reads it.
 *   inflation (uint32)d < n_curve ? curve[d] : 0.  Never unknown: PWPP_DIST_BEYOND and any negative word read 0.
 *   terrain   t < 0 is unknown; t > 100 counts as 100; otherwise the value is t.
 *   unknown   An unknown occupancy value becomes occupancy_unknown if that is >= 0 and otherwise stays unknown; an unknown terrain
 *             value likewise with terrain_unknown.
 *   fold      m = the maximum of the known values of the enabled layers, or 0 if none is known.  cost = -1 if some enabled layer
 *             is still unknown and m < unknown_below; otherwise cost = m.  unknown_below 101: unknown always wins; 100: a lethal
 *             cell shows through an unknown one; 1: any positive cost does.  cost is in pwpp_reach_grid's input range:
 *             lethal = 100 blocks the obstacles, `unknown` handles -1.
 *   why       optional uint8 image: bits 1, 2 and 4 are set for each enabled layer whose known value equals m, when m > 0; bit 8
 *             (PWPP_COSTMAP_WHY_UNKNOWN) iff some enabled layer stayed unknown.  It does not depend on whether cost came out -1.
 *   own distances  PWPP_COSTMAP_INFLATION with dist2 == NULL (pwpp_costmap_grid): occupancy must be given and is read for this
 *             purpose even where PWPP_COSTMAP_OCCUPANCY is not among the layers.  The call widens (o == PWPP_OCC_OCCUPIED) to an
 *             int32 count image in the cluster buffer and runs pwpp_distance_grid's kernels on it with min_count 1 and max_dist =
 *             max(1, R), R the least integer with R * R >= n_curve - 1.  The result is byte for byte that of passing the uncapped
 *             dist2: every value the cap turns into PWPP_DIST_BEYOND exceeds n_curve - 1 and reads 0 either way.  A fused
 *             map_occupancy becomes a costmap this way without leaving the device (sides <= 32768 as for every distance).
 *   costmap_obstacles  one enqueued sequence for frames of the LAST estimate call, only the stages the enabled layers need:
 *             pwpp_rasterize_obstacles (OCCUPANCY or INFLATION); the visibility's byte (OCCUPANCY: origin_xy, n_origins and
 *             max_range as pwpp_visibility_obstacles takes them, otherwise not read); the distances with the cap above from the
 *             COUNT image and min_count (INFLATION: what pwpp_distance_obstacles gives with that max_dist; the inflation reads the
 *             same bytes off the uncapped image); pwpp_rasterize_ground and the terrain's cost alone (TERRAIN: terrain_params as
 *             pwpp_terrain_ground takes them, NULL allowed otherwise); the fold.  occupancy, dist2 and terrain are written for the
 *             caller where asked for and their layer ran, kept in the handle's cluster buffer otherwise; each is exactly what the
 *             stand-alone call gives.  Before any estimate call: PWPP_E_STATE.  The call does not run the reach: pwpp_reach_grid
 *             on the device cost image right after it, on the same stream with no synchronise between, is the planner's chain.
 *   mem       PWPP_MEM_HOST: every image is host memory, staged through the handle's cluster buffer; synchronous.
 *             PWPP_MEM_DEVICE: device memory -- dist2 4-byte aligned, every byte image at any address, each at its own --
 *             enqueued on the handle's stream, complete after pwpp_synchronize.  PWPP_MEM_HOST_PINNED: PWPP_E_ARG.
 *   errors    PWPP_E_ARG, named before the device is touched, in this order.  pwpp_costmap_grid: a null handle, parameters, cost;
 *             frames or a side < 1, a side > 32768, nx * ny * frames beyond 2^31; layers, occupancy_unknown, terrain_unknown,
 *             unknown_below, pad_; with INFLATION a null curve, n_curve outside 1 .. 4097, the first entry above 100; the image
 *             of an enabled layer that is null -- occupancy (also: INFLATION without dist2), then terrain; two of the caller's
 *             images overlapping; mem; in PWPP_MEM_DEVICE a dist2 below its alignment.  pwpp_costmap_obstacles: a null handle,
 *             grid, parameters, cost; the parameters and the curve as above; with OCCUPANCY a null origin, with TERRAIN null
 *             terrain parameters; frames or a side < 1, a side > 32768, g->flags other than 0 or PWPP_GRID_GROUND_ONLY; with
 *             OCCUPANCY or INFLATION the height band and min_count; with OCCUPANCY the grid's origin and cell, max_range, the
 *             count of origins, then the first that is not finite or lies outside the grid; with TERRAIN the terrain parameters
 *             as pwpp_terrain_ground names them; the overlaps; then what pwpp_rasterize_ground checks -- the grid's origin and
 *             cell, mem, PWPP_E_STATE before any estimate call, the frame range, the product beyond 2^31 -- and the alignment.
 *   buffers   The uploaded table (at most 1025 words), the count image and the distance kernels' working image of the own
 *             distances, the chain's kept images and in PWPP_MEM_HOST the staged images lie in the cluster buffer; counted by
 *             pwpp_get_workspace_bytes, freed by pwpp_trim_workspace.  pwpp_costmap_grid needs a handle for its stream and this
 *             buffer only.
 *   host only pwpp_costmap_cell is the rule for one cell, compiled from the text the kernels are compiled from: o and t are read
 *             as int8 values, cost and why may each be NULL; the parameters and the curve are checked as above.
 *             pwpp_costmap_curve fills a common table: cell > 0, 0 <= inscribed <= radius, decay >= 0, all finite, peak 0 .. 99.
 *             n_curve - 1 is the largest integer d with sqrt((double)d) * cell <= radius, and radius / cell beyond 64 is
 *             PWPP_E_ARG; curve[d] = 100 where sqrt(d) * cell <= inscribed, otherwise (int)floor(peak * exp(-decay * (sqrt(d) *
 *             cell - inscribed))), with the C library's exp.  Returns n_curve, or PWPP_E_ARG (capacity < n_curve included).  The
 *             table it returns is what the device is handed and is the contract; the helper is a convenience.
 * The same bytes for every mem, alignment and value of the option "costmap_path".  With none of these functions called nothing is
 * allocated or launched, and no result, state or timing of any other call changes. */
#define PWPP_HAS_COSTMAP 1
#define PWPP_COSTMAP_OCCUPANCY 1
#define PWPP_COSTMAP_INFLATION 2
#define PWPP_COSTMAP_TERRAIN   4
#define PWPP_COSTMAP_WHY_UNKNOWN 8
#define PWPP_COSTMAP_MAX_CURVE 4097
typedef struct pwpp_costmap_params {   /* 24 bytes */
    int32_t layers;             /* a mask of PWPP_COSTMAP_OCCUPANCY, _INFLATION, _TERRAIN; not 0 */
    int32_t occupancy_unknown;  /* -1: an unknown occupancy byte stays unknown; 0 .. 100: it counts as this value */
    int32_t terrain_unknown;    /* the same for a terrain byte < 0 */
    int32_t unknown_below;      /* a cell with an unknown layer is -1 unless its maximum reaches this; 1 .. 101 */
    int32_t pad_[2];            /* 0 */
} pwpp_costmap_params;

/* any images: needs a handle (stream, buffer), no estimate call -- like pwpp_reach_grid */
PWPP_API int pwpp_costmap_grid(pwpp_handle *h, int nx, int ny, int frames, int mem, const int8_t *occupancy /* [frames][ny][nx], may be NULL */,
                               const int8_t *terrain /* same shape, may be NULL */, const int32_t *dist2 /* same shape, may be NULL */,
                               const pwpp_costmap_params *p, const uint8_t *curve /* host: n_curve entries */, int n_curve,
                               int8_t *cost /* same shape */, uint8_t *why /* same shape, may be NULL */);
/* the layers' stages and the fold for frames of the LAST estimate call, one enqueued sequence -- like pwpp_reach_ground */
PWPP_API int pwpp_costmap_obstacles(pwpp_handle *h, const pwpp_ground_grid *g /* flags: 0 or PWPP_GRID_GROUND_ONLY */, float h_min, float h_max, int min_count,
                                    const double *origin_xy /* host: n_origins x {x, y}, metres */, int n_origins, int max_range,
                                    const pwpp_terrain_params *terrain_params, const pwpp_costmap_params *p, const uint8_t *curve, int n_curve,
                                    int frame_first, int frames, int mem, int8_t *cost, uint8_t *why /* may be NULL */,
                                    int8_t *occupancy /* may be NULL: kept */, int32_t *dist2 /* may be NULL: kept */, int8_t *terrain /* may be NULL: kept */);
PWPP_API int pwpp_costmap_cell(const pwpp_costmap_params *p, const uint8_t *curve, int n_curve, int o, int t, int32_t d,
                               int32_t *cost, uint32_t *why);   /* host only */
PWPP_API int pwpp_costmap_curve(double cell, double inscribed, double radius, double decay, int peak /* 0 .. 99 */,
                                uint8_t *curve, int capacity);  /* host only; returns n_curve */

/* ---- routes: the from chain of the reach field walked, summarised and shortcut on the device (pwpp_route_grid, pwpp_plan_grid) ----
 * pwpp_reach_grid gives every cell its cost and the neighbour it comes through; a controller wants the way itself: which cells,
 * how long, how close to an obstacle, how dear at its worst, and the few waypoints a tracker follows instead of a staircase of
 * cells.  These calls follow `from` on the device for any number of starts per frame and return a row of 32 bytes, the cells and
 * the waypoints per route -- the from image (4 bytes a cell) never has to reach the host.  Integers only: the same bytes whatever
 * the schedule.  Frames, and the routes of a frame, are on their own.
 *   terms, steps  exactly those of pwpp_reach_grid (above): the same cost, dist2, pwpp_reach_params and corner rule give t(cell) and
 *             step(a, b); max_reach is not read.  The frame's source has its term wherever it is read -- on a line that merely passes
 *             over it too.  The range check of pwpp_reach_grid applies: every sum below stays under 2^31.
 *   route     of a start s: r_0 = s, r_{i+1} = from[r_i], ending at the cell that names itself, which must be the frame's source.
 *             Every list runs in this order, from the start to the source.  step is symmetric: a caller who wants "vehicle to
 *             goal" puts the field's source at the goal and the start at the vehicle, and reads the lists as they are.
 *   status    PWPP_ROUTE_NONE: from[s] == -1.  Every other field of the row is 0, min_dist2 is PWPP_DIST_BEYOND, both lists are all -1.
 *             PWPP_ROUTE_BROKEN: a hop from c to n = from[c] is not a step of the contract -- n outside [0, nx ny); n not one of
 *             the 8 neighbours of c; n == c away from the source (the chain ends at a cell other than the source); t(c) or t(n)
 *             is 0; a cut corner; or nx ny - 1 hops were taken without arriving.  The row then holds what the valid hops up to c
 *             accumulated: `cells` counts up to and including c, max_term and min_dist2 cover those cells, the cell list holds that
 *             prefix, `waypoints` is 0 and its list all -1.  A from image of pwpp_reach_grid on the same inputs never gives
 *             PWPP_ROUTE_BROKEN.  The hop bound is the only loop bound of the walk; no kernel loops on past it.
 *             PWPP_ROUTE_OK: otherwise.  Then cost == reach[s].
 *   lists     The cell list of a route holds its first min(cells, max_cells) indices iy * nx + ix and -1 behind them; the waypoint
 *             list the same with max_waypoints.  The row's counts are of the whole route: cells > max_cells is how a caller sees a
 *             truncation.  Neither limit changes any other value.  A limit of 0: no list, the pointer may be NULL.
 *   waypoints indices into the route: w_0 = 0; from w_i = a < cells - 1, w_{i+1} is the largest b in (a, min(a + look, cells - 1)]
 *             for which b == a + 1 or the line r_a -> r_b is clear.  The line is that of the visibility operator (above), from the
 *             earlier cell to the later: with n = max(|dx|, |dy|) the points P_k, k = 0 .. n.  It is clear iff for every k = 1 .. n:
 *             0 < t(P_k) <= base + line_cost, and wherever both coordinates moved both cells the step squeezes between have t > 0
 *             -- the reach's corner rule, stricter than the visibility's.  The last waypoint is the source.  Stored waypoints are
 *             cell indices.  It follows that the polyline, rasterised by the same line, is a legal step path of the reach contract
 *             from the start to the source; that look = 1 returns the route itself; and that on an open field of one cost byte
 *             <= line_cost with look >= cells - 1 every route has 2 waypoints, 1 where the start is the source.  max_waypoints
 *             == 0: no search, `waypoints` of the row is 0.  (csrc/pwpp_route.h has the proofs.)
 *   row       status; cells; cost, the sum of the steps; edge_steps and corner_steps (the length in metres is cell * (edge_steps +
 *             sqrt(2) corner_steps), left to the caller: no floating point here); max_term, the largest t over the cells;
 *             min_dist2, the smallest dist2 over them (PWPP_DIST_BEYOND without a dist2 image); waypoints.
 *   starts    n_start_sets x n_starts x {x, y} cells, host memory whatever `mem`, copied at the call, like the sources;
 *             n_start_sets is 1 (one set for every frame) or `frames`; n_starts 1 .. 65536; frames * n_starts * max(max_cells,
 *             max_waypoints, 1) <= 2^31 - 1.  Starts may repeat and may be the source.
 *   plan_grid pwpp_reach_grid and pwpp_route_grid on its from as one enqueued sequence: byte for byte what the two calls give.
 *             reach and from may be NULL and then stay in the handle's buffer: the field never leaves the device.
 *   mem       as pwpp_reach_grid: PWPP_MEM_DEVICE asks 4-byte alignment of dist2, reach, from, the rows and both lists; the cost
 *             bytes lie at any address.
 *   errors    PWPP_E_ARG, named before the device is touched, in this order: a null handle, cost, reach parameters, source, from
 *             (pwpp_route_grid), start, route parameters, routes; then what pwpp_reach_grid checks of the images, its parameters,
 *             the range and the sources; max_cells, max_waypoints, look, line_cost; the count of start sets, of starts, the product
 *             beyond 2^31 - 1; the first start outside the image, naming the entry; a null list with its limit > 0; two of the
 *             caller's arrays overlapping; mem; in PWPP_MEM_DEVICE an int32 array below its alignment.
 *   buffers   The uploaded starts and sources, in pwpp_plan_grid the reach's working memory and the images the caller did not ask
 *             for, and in PWPP_MEM_HOST the staged arrays lie in the cluster buffer; counted by pwpp_get_workspace_bytes, freed
 *             by pwpp_trim_workspace.
 * The same bytes for every mem, alignment and value of the option "route_path".  With neither function called nothing is
 * allocated or launched, and no result, state or timing of any other call changes. */
#define PWPP_HAS_ROUTES 1
#define PWPP_ROUTE_OK 0
#define PWPP_ROUTE_NONE 1
#define PWPP_ROUTE_BROKEN 2
typedef struct pwpp_route_params {   /* 16 bytes */
    int32_t max_cells;      /* cells stored per route, >= 0 (0: no cell list; `cells` may be NULL) */
    int32_t max_waypoints;  /* waypoints stored per route, >= 0 (0: no shortcut search; `waypoints` may be NULL) */
    int32_t look;           /* how many cells ahead a shortcut may reach; 1 .. 256 */
    int32_t line_cost;      /* a shortcut line crosses only cells with t <= base + line_cost; 0 .. 100 */
} pwpp_route_params;
typedef struct pwpp_route {          /* 32 bytes: one row per (frame, start) */
    int32_t status;        /* PWPP_ROUTE_OK, PWPP_ROUTE_NONE, PWPP_ROUTE_BROKEN */
    int32_t cells;         /* cells of the whole route, start and source included, whatever max_cells */
    int32_t cost;          /* the sum of the steps along it: equals reach[start] */
    int32_t edge_steps, corner_steps;
    int32_t max_term;      /* the largest t over its cells */
    int32_t min_dist2;     /* the smallest dist2 over its cells; PWPP_DIST_BEYOND without a dist2 image */
    int32_t waypoints;     /* waypoints of the whole route, whatever max_waypoints; 0 with max_waypoints == 0 */
} pwpp_route;

/* follow a given from image: needs a handle (stream, buffer), no estimate call -- like pwpp_reach_grid */
PWPP_API int pwpp_route_grid(pwpp_handle *h, int nx, int ny, int frames, int mem, const int8_t *cost /* [frames][ny][nx] */,
                             const int32_t *dist2 /* same shape, may be NULL */, const pwpp_reach_params *p,
                             const int32_t *source /* host: n_sources x {sx, sy} */, int n_sources /* 1 or frames */,
                             const int32_t *from /* same shape: of pwpp_reach_grid */,
                             const int32_t *start /* host: n_start_sets x n_starts x {x, y} */, int n_start_sets /* 1 or frames */, int n_starts,
                             const pwpp_route_params *route_params, pwpp_route *routes /* [frames][n_starts] */,
                             int32_t *cells /* [frames][n_starts][max_cells] */, int32_t *waypoints /* [frames][n_starts][max_waypoints] */);
/* cost image -> field -> routes, one enqueued sequence */
PWPP_API int pwpp_plan_grid(pwpp_handle *h, int nx, int ny, int frames, int mem, const int8_t *cost, const int32_t *dist2, const pwpp_reach_params *p,
                            const int32_t *source, int n_sources, const int32_t *start, int n_start_sets, int n_starts,
                            const pwpp_route_params *route_params, pwpp_route *routes, int32_t *cells, int32_t *waypoints,
                            int32_t *reach /* may be NULL: kept in the handle's buffer */, int32_t *from /* may be NULL: kept */);

/* ---- oriented vehicle footprint: poses checked and trajectories scored against the cost image on the device (pwpp_footprint_grid) ----
 * The costmap's inflation, the reach's clearance2 and a route's min_dist2 all speak of a point with a round collar.  A car of 4.5 m x
 * 1.8 m has an inscribed radius of 0.9 m and a circumscribed one of about 2.4 m; whether a cell between them is free depends on the
 * heading.  This call lays the vehicle's rectangle over the cost image at every pose of a fan of candidate trajectories and returns a
 * row of 32 bytes per pose and per trajectory -- cost, dist2 and reach never have to reach the host.  Integers only, no angle: a
 * heading is an integer vector.  The same bytes whatever the schedule.  Frames, and the trajectories of a frame, are on their own.
 *   ticks     A tick is 1/PWPP_FOOT_SUB = 1/16 of a cell side.  Cell (ix, iy) covers the ticks [16 ix, 16 ix + 16) in x, [16 iy, 16 iy + 16)
 *             in y; its centre is q = (16 ix + 8, 16 iy + 8).  Tick coordinates may be negative or lie beyond the image.
 *   pose      {px, py, ux, uy}: the reference point p in ticks, |px|, |py| <= 2^20; the heading u, any integer vector with |ux|, |uy| <=
 *             1024, of which only the direction matters.  u == (0, 0) is no pose: status PWPP_FOOT_SKIPPED -- how ragged trajectories
 *             are padded.
 *   footprint the rectangle [-rear, front] along u and [-half_width, half_width] across it, in ticks, each of the three 0 ..
 *             PWPP_FOOT_MAX_EXTENT (64 cells, the costmap's largest radius); rear != front puts p on a rear axle.
 *   covered   With d = q - p, a = ux dx + uy dy, b = ux dy - uy dx, n2 = ux^2 + uy^2, all in int64: a cell is covered iff
 *             (a >= 0 ? a^2 <= front^2 n2 : a^2 <= rear^2 n2) and b^2 <= half_width^2 n2.  Equality is inside.
 *             Lemma 1: a covered cell has max(|dx|, |dy|) <= max(front, rear) + half_width <= 2048; only that window is visited and
 *             every product stays below 2^45.  Lemma 2: a footprint padded by 12 ticks on every side covers every cell that the
 *             unpadded rectangle touches at all (8 sqrt(2) < 12): the caller's knob for a conservative check.  (csrc/pwpp_footprint.h
 *             has the proofs.)
 *   pose row  over the pose's covered cells: `covered`, all of them, inside the image or not; `outside`, those with ix or iy outside
 *             the image (no address is formed for them).  For the covered cells inside, t = the term of the reach contract (above)
 *             from the same cost, dist2 and pwpp_reach_params, with no source exception: `blocked`, the count with t == 0; `unknown`,
 *             the count with a cost byte < 0, whatever p->unknown substitutes; max_term, the largest t (0 without one); min_dist2,
 *             the smallest dist2 over all of them, blocked ones too (PWPP_DIST_BEYOND without a dist2 image or without such a cell);
 *             `hit`, the smallest index iy nx + ix of a blocked cell, or -1.  status: PWPP_FOOT_HIT iff blocked > 0, or outside > 0
 *             with PWPP_FOOT_OUTSIDE_BLOCKS in flags; else PWPP_FOOT_FREE.  A skipped pose's row is {PWPP_FOOT_SKIPPED, 0, 0, 0, 0, 0,
 *             PWPP_DIST_BEYOND, -1}.  max_reach of p is not read.
 *   traj row  of frame f and trajectory j, over the poses of set 0 or of set f: first_hit, the smallest step whose status is HIT, or
 *             -1.  The free prefix: the steps that are not skipped and lie before first_hit (all that are not skipped without one).
 *             free_steps, its size; `last`, its largest step, or -1; max_term and sum_term, the maximum and the sum of its poses'
 *             max_term; `unknown`, the sum of their unknown; min_dist2, the minimum of theirs; reach_last, reach[f] at the cell
 *             (px >> 4, py >> 4) of pose `last` (an arithmetic shift) where reach was given, last >= 0 and that cell lies inside, else
 *             PWPP_REACH_NONE.  With 4096 steps every sum stays below 2^31 (355 x 4096; 66049 x 4096).  Every field is a min, a max,
 *             a sum or an ordered pick: the same bytes whatever the deal.
 *   limits    n_sets 1 or `frames`; n_traj 1 .. 65536; n_steps 1 .. PWPP_FOOT_MAX_STEPS; frames x n_traj x n_steps <= 2^26; the sides,
 *             the frames and their product as pwpp_reach_grid has them.  The range check of pwpp_reach_grid is not made: nothing is
 *             summed over the image.
 *   mem       as pwpp_route_grid: PWPP_MEM_HOST stages every array through the cluster buffer and returns when the rows are there;
 *             PWPP_MEM_DEVICE enqueues on the handle's stream, the cost bytes lie at any address, dist2, reach and both row arrays are
 *             4-byte aligned.  `poses` is host memory whatever `mem` and is copied at the call.  PWPP_MEM_HOST_PINNED: PWPP_E_ARG.
 *   errors    PWPP_E_ARG, named before the device is touched, in this order: a null handle, cost, reach parameters, footprint
 *             parameters, poses; the image's shape; the reach parameters as pwpp_reach_grid names them, without the range; front,
 *             rear, half_width, unknown flag bits, pad_ not 0; the count of sets, of trajectories, of steps, their product beyond
 *             2^26; the first pose entry out of range, naming set, trajectory and step; both row arrays null; two of the caller's
 *             arrays overlapping; mem; in PWPP_MEM_DEVICE an int32 array below its alignment.
 *   buffers   The uploaded poses, in PWPP_MEM_HOST the staged arrays and on "footprint_path" 1 the pose rows of a call that asks for
 *             trajectory rows alone lie in the cluster buffer; counted by pwpp_get_workspace_bytes, freed by pwpp_trim_workspace.
 *   helpers   pwpp_footprint_covers: the coverage rule itself for any cell, 1 or 0 (PWPP_E_ARG: a null pointer, parameters or a pose
 *             out of range; u == (0, 0) covers nothing).  pwpp_footprint_pose: a convenience, not the contract: px = (int)floor((x -
 *             g->x0) / g->cell * 16), py alike, ux = lround(1024 cos yaw), uy = lround(1024 sin yaw); PWPP_E_ARG for a value that is
 *             not finite or a p beyond 2^20.
 * The same bytes for every mem, alignment and value of the option "footprint_path".  With the function never called nothing is
 * allocated or launched, and no result, state or timing of any other call changes. */
#define PWPP_HAS_FOOTPRINT 1
#define PWPP_FOOT_SUB 16            /* ticks per cell side */
#define PWPP_FOOT_MAX_EXTENT 1024   /* ticks: 64 cells, the costmap's largest radius */
#define PWPP_FOOT_MAX_STEPS 4096
#define PWPP_FOOT_FREE 0
#define PWPP_FOOT_HIT 1
#define PWPP_FOOT_SKIPPED 2
#define PWPP_FOOT_OUTSIDE_BLOCKS 1  /* flags */
typedef struct pwpp_footprint_params { int32_t front, rear, half_width, flags, pad_[2]; } pwpp_footprint_params;   /* 24 bytes */
typedef struct pwpp_footprint_pose_row { int32_t status, covered, outside, blocked, unknown, max_term, min_dist2, hit; } pwpp_footprint_pose_row;       /* 32 bytes */
typedef struct pwpp_footprint_traj_row { int32_t first_hit, free_steps, last, max_term, sum_term, unknown, min_dist2, reach_last; } pwpp_footprint_traj_row; /* 32 bytes */

/* needs a handle (stream, buffer), no estimate call -- like pwpp_route_grid */
PWPP_API int pwpp_footprint_grid(pwpp_handle *h, int nx, int ny, int frames, int mem,
        const int8_t *cost /* [frames][ny][nx] */, const int32_t *dist2 /* same shape, may be NULL */,
        const int32_t *reach /* same shape, may be NULL */, const pwpp_reach_params *p, const pwpp_footprint_params *fp,
        const int32_t *poses /* HOST: [n_sets][n_traj][n_steps][4] = {px, py, ux, uy} */, int n_sets /* 1 or frames */, int n_traj, int n_steps,
        pwpp_footprint_pose_row *pose_rows /* [frames][n_traj][n_steps], may be NULL */,
        pwpp_footprint_traj_row *traj_rows /* [frames][n_traj], may be NULL; not both NULL */);
PWPP_API int pwpp_footprint_covers(const pwpp_footprint_params *fp, const int32_t pose[4], int ix, int iy);  /* host only: 1, 0 or PWPP_E_ARG */
PWPP_API int pwpp_footprint_pose(const pwpp_ground_grid *g, double x, double y, double yaw, int32_t pose[4]); /* host only, a convenience */

/* ---- viewshed: line of sight that sees over low obstacles, with ground returns (pwpp_viewshed_grid, pwpp_viewshed_obstacles) ----
 * pwpp_visibility_* (above) stops a line at the first occupied cell, however low: every kerb, bollard and parked car throws a shadow
 * to the edge of the grid although the sensor, mounted above them, saw the road behind.  This operator walks the SAME digital line
 * with heights: an occupied cell hides a cell behind it only if the ray from the eye to that cell's ground (or top) passes through
 * it; and a cell whose ground sent a return back is free whatever the line says.  Per cell, integers only, each frame on its own,
 * the same bytes whatever the schedule.  The upstream Patchwork++ has nothing of this kind.
 *   heights   int32, all in one unit with the vertical origin of the caller's choice; PWPP_VIEW_NO_HEIGHT (INT32_MIN) is "none".
 *             R = PWPP_VIEW_MAX_RISE = 2^20.
 *   origin    {ox, oy, eye} per frame: the sensor's cell, inside the image, and its height.  HOST memory in both mem kinds, n_origins
 *             1 or `frames`, copied at the call like the origins of pwpp_visibility_grid.  eye == PWPP_VIEW_NO_HEIGHT: PWPP_E_ARG,
 *             naming the entry.
 *   cells     A cell is occupied iff count >= min_count.  An occupied cell has the blocker rise clamp(block - eye, -R, R), computed in
 *             64 bits; one whose block is PWPP_VIEW_NO_HEIGHT, and every occupied cell when `block` is NULL, is OPAQUE.  A cell's
 *             target rise t is that of `block` where the cell is occupied (is its top seen?), else that of `target`, clamped alike; a
 *             height of PWPP_VIEW_NO_HEIGHT, or a NULL image, counts as minus infinity.
 *   walk      The line and its points P_k, k = 0 .. n, are those of pwpp_visibility_grid.  At step k = 1 .. n, in this order:
 *             (a) if both coordinates changed and A = (x_{k-1}, y_k) and B = (x_k, y_{k-1}) are both occupied, the gap between them
 *             is a blocker at D = 2k - 1 whose rise is the smaller of the two rises -- a finite rise counts as below opaque -- and
 *             whose reported cell is the one with the smaller rise, on equal rises the smaller index; (b) for k < n only: if P_k is
 *             occupied it is a blocker at D = 2k with its own rise.  The cell's own returns never hide the cell itself, and the
 *             origin's cell never blocks.
 *   hides     A blocker (r, D) hides the target iff it is opaque, or t is minus infinity, or r * 2n > t * D.  Strict: a grazing ray
 *             sees.  Every product stays below 2^38.
 *   first     In this order: PWPP_VIS_BEYOND if n > max_range > 0 (nothing on the line is read then); the reported cell of the NEAREST
 *             blocker that hides; the cell's own index if it is occupied; PWPP_VIS_NONE.
 *   shadow    (may be NULL) the lowest height seen at the cell: PWPP_VIEW_NO_HEIGHT when the line has no blocker or the cell is
 *             beyond range; INT32_MAX behind an opaque blocker; otherwise eye + clamp(max over the blockers b of
 *             ceil(r_b * 2n / D_b), -R, R + 1), the division exact (a sum beyond the int32 range saturates at INT32_MIN + 1 and
 *             INT32_MAX - 1: only with |eye| > 2^31 - 2^20 - 2).  THEOREM: a cell whose line has a blocker is hidden iff its target rise
 *             < shadow - eye (minus infinity is below everything, INT32_MAX above).
 *   occupancy (may be NULL) in this order: PWPP_OCC_OCCUPIED where the cell is occupied; else PWPP_OCC_FREE where `seen` is given and
 *             seen >= min_seen -- a WITNESSED cell: a return came back from its ground; it holds beyond max_range too; else
 *             PWPP_OCC_FREE where first == PWPP_VIS_NONE; else PWPP_OCC_UNKNOWN.
 *   THEOREMS  1. With block, target and seen NULL, first and occupancy are byte for byte those of pwpp_visibility_grid: every blocker
 *             is opaque and hides, rule (b) at k = n is the cell's own index.  2. For any heights the FREE cells of
 *             pwpp_visibility_grid are a subset of this operator's: a line without an occupied cell has no blocker.  3. max_range
 *             changes no value inside it.  4. A kerb of height 1500 at cell 4 of a row, seen from cell 0 with eye 1700 over ground 0
 *             (r = -200, t = -1700, D = 8: hidden iff 400 n < 13600), hides exactly the cells 5 .. 33; shadow is 1200 at cell 10 and 0
 *             at cell 34.
 *   units     pwpp_viewshed_units, the quantiser of the chained call, PWPP_VIEW_UNITS_PER_M = 1024: PWPP_VIEW_NO_HEIGHT for a NaN,
 *             otherwise floor(clamp(metres * 1024.0, -2^30, 2^30) + 0.5), in double.
 *   ground_returns   seen[f][iy][ix] = the points the frame's GROUND index list names that fall into the cell, by the cell rule of
 *             pwpp_rasterize_obstacles on the same INPUT; when, mem, the lifetime rule and the errors are that function's, except
 *             that g->flags must be 0 (there is no reference to blank).  Integer adds: a function of the input alone.
 *   viewshed_obstacles   enqueues, on the handle's stream: the obstacle raster (count, top) of pwpp_rasterize_obstacles(g, h_min, h_max,
 *             ...); the ground raster of pwpp_rasterize_ground on the same grid (g->flags 0 or PWPP_GRID_GROUND_ONLY); where min_seen >
 *             0 the ground-returns raster (min_seen == 0: no `seen`; it reads no flags); and pwpp_viewshed_grid with target =
 *             units(ground), block = units((double)ground + (double)top), eye = units(z) of the origin {x, y, z} in metres, x and y
 *             turned into a cell as pwpp_visibility_obstacles turns them.  The quantiser runs on the device, the same function: a NaN
 *             ground gives an opaque blocker and a target at minus infinity -- the 2-D answer, the conservative side.  The images
 *             are exactly what the four calls give one after the other.
 *   mem       as pwpp_visibility_grid: PWPP_MEM_HOST stages every image through the handle's cluster buffer, synchronous;
 *             PWPP_MEM_DEVICE: device memory, the int32 images 4-byte aligned and no more, occupancy byte aligned, enqueued on the
 *             handle's stream.  PWPP_MEM_HOST_PINNED: PWPP_E_ARG.
 *   errors    pwpp_viewshed_grid: PWPP_E_ARG, named before the device is touched, in this order: a null handle, count, first or
 *             origin; nx, ny or frames < 1; nx or ny > 32768; nx * ny * frames beyond 2^31; min_count < 1; max_range outside 0 ..
 *             32768; min_seen < 1 with a non-null seen; the number of origins; an origin outside the image; an eye that is
 *             PWPP_VIEW_NO_HEIGHT; mem.  pwpp_viewshed_obstacles: a null handle, grid, first or origin; everything
 *             pwpp_visibility_obstacles rejects up to max_range; min_seen < 0; the number of origins; an origin that is not finite
 *             (z included) or outside the grid; then what pwpp_rasterize_obstacles rejects of the frame range and mem;
 *             PWPP_E_STATE before any estimate call.
 *   buffers   The bit image of "viewshed_path" 2 (one bit per cell, rows padded to 32), the origins where there is one per frame, in
 *             PWPP_MEM_HOST the staged images and in the chained call its five intermediate images lie in the cluster buffer:
 *             counted by pwpp_get_workspace_bytes, freed by pwpp_trim_workspace.
 * pwpp_fuse_obstacles, pwpp_match_obstacles and pwpp_costmap_obstacles keep the 2-D bytes of pwpp_visibility_obstacles; feed these
 * bytes to pwpp_fuse_grid, pwpp_match_grid and pwpp_costmap_grid instead.  The same bytes for every mem, alignment
 * and value of the option "viewshed_path".  With none of the functions called nothing is allocated or launched, and no result, state
 * or timing of any other call changes. */
#define PWPP_HAS_VIEWSHED 1
#define PWPP_VIEW_NO_HEIGHT (-2147483647 - 1)   /* INT32_MIN: no height */
#define PWPP_VIEW_MAX_RISE 1048576              /* R = 2^20 units */
#define PWPP_VIEW_UNITS_PER_M 1024

/* any images: needs a handle (stream, buffer), no estimate call -- like pwpp_visibility_grid */
PWPP_API int pwpp_viewshed_grid(pwpp_handle *h, int nx, int ny, int frames, int mem,
                                const int32_t *count /* [frames][ny][nx] */, int min_count,
                                const int32_t *block /* same shape, may be NULL */, const int32_t *target /* same shape, may be NULL */,
                                const int32_t *seen /* same shape, may be NULL */, int min_seen,
                                const int32_t *origin /* HOST memory, n_origins x {ox, oy, eye} */, int n_origins,
                                int max_range /* cells, Chebyshev; 0: unlimited */,
                                int32_t *first /* [frames][ny][nx] */, int32_t *shadow /* same shape, may be NULL */,
                                int8_t *occupancy /* same shape, may be NULL */);
/* the ground list of frames of the LAST estimate call per cell -- like pwpp_rasterize_obstacles */
PWPP_API int pwpp_rasterize_ground_returns(pwpp_handle *h, const pwpp_ground_grid *g, int frame_first, int frames, int mem,
                                           int32_t *seen /* [frames][ny][nx] */);
/* both rasters + ground returns + viewshed for frames of the LAST estimate call, one call -- like pwpp_visibility_obstacles */
PWPP_API int pwpp_viewshed_obstacles(pwpp_handle *h, const pwpp_ground_grid *g, float h_min, float h_max,
                                     int min_count, int min_seen, const double *origin_xyz /* HOST, n_origins x {x, y, z} metres */,
                                     int n_origins, int max_range, int frame_first, int frames, int mem,
                                     int32_t *first, int32_t *shadow /* may be NULL */, int8_t *occupancy /* may be NULL */,
                                     int32_t *count /* may be NULL: kept */);
PWPP_API int32_t pwpp_viewshed_units(double metres);   /* host only: the quantiser */

/* ---- per-beam free space: every return's ray traced through the grid (pwpp_rasterize_beams, pwpp_beam_grid, pwpp_beam_ground) ----
 * The two lines of sight above decide on the obstacle image whether a cell COULD be seen.  A return is stronger evidence: its whole
 * beam, from the sensor to the point, went through empty air, so every cell under the beam has been measured empty above the beam's
 * height at that cell.  This stage draws the beam of every endpoint cell along the visibility's digital line and reports, per crossed
 * cell, how many beams passed and the lowest of them -- the free space behind a hedge the sensor saw over, or between two parked
 * cars, which both lines of sight leave PWPP_OCC_UNKNOWN.  Integers only, each frame on its own, the same bytes whatever the
 * schedule.  The upstream Patchwork++ has nothing of this kind.
 *   rasterize_beams   the endpoints of the LAST call's beams on the grid g (flags must be 0): when, frame_first, frames, mem, the lifetime
 *             rule of the input and the errors are those of pwpp_rasterize_ground_returns.  `which`: bit 1 selects the frame's ground
 *             list, bit 2 its non-ground list; 0 or any other bit: PWPP_E_ARG.  hits[f][iy][ix] = the selected points that fall into
 *             the cell, by the cell rule of pwpp_rasterize_obstacles on the same INPUT (input transforms apply); zmin = the smallest
 *             pwpp_viewshed_units((double)z) among them, PWPP_VIEW_NO_HEIGHT where there is none.  A point whose z is a NaN is skipped
 *             and not counted; a point outside the grid is skipped.  Integer adds and minima: a function of the input alone.
 *             NOTE: the non-ground list also holds the points the reflected-noise removal rejected.  Their beams end BELOW the
 *             ground -- they would clear cells the sensor never saw through -- so which = 1 is the safe default.
 *   endpoints A cell e is an endpoint iff hits[e] >= 1 and zmin[e] != PWPP_VIEW_NO_HEIGHT; its beam has the weight hits[e] and the
 *             height zmin[e].
 *   origin    {ox, oy, eye} per frame, as pwpp_viewshed_grid takes it: HOST memory in both mem kinds, n_origins 1 or `frames`.  |eye| <=
 *             2^30, so that `low` can never leave int32.
 *   line      The points P_k, k = 0 .. n, from the origin's cell to e are those of pwpp_visibility_grid.  The beam CROSSES the interior
 *             points P_1 .. P_{n-1}: the origin's cell holds the vehicle, the endpoint's cell the return.  An endpoint with n <= 1
 *             crosses nothing.  Occupied cells do not stop a beam: a beam that returned did pass.
 *   height    at a crossed cell P_k: r = clamp(zmin[e] - eye, -R, R) in 64 bits, R = PWPP_VIEW_MAX_RISE; D = 2k - 1 where r < 0, else
 *             2k + 1 -- the end of the cell's stretch of the beam where the beam is highest, so that what the cell reports is an
 *             upper bound over the whole cell; height = eye + ceil(r * D / (2n)), the division exact.  Every product stays below 2^37.
 *             pwpp_beam_height(eye, z, k, n) is this rule on the host, compiled from the text the kernels are compiled from
 *             (1 <= k < n <= 32768, |eye| <= 2^30, z a height; otherwise PWPP_VIEW_NO_HEIGHT and the error text).
 *   passes    passes[c] = the sum of the weights of the beams that cross c, in unsigned 32-bit arithmetic (it wraps).
 *   low       low[c] = the smallest height among those beams; PWPP_VIEW_NO_HEIGHT where passes[c] == 0.
 *   THEOREM   For fixed k and n the height is non-decreasing in z.  So the lowest of many beams into one endpoint cell is the beam of
 *             its lowest point, and tracing every POINT's beam from its own cell and z gives exactly these two images: hits and zmin
 *             lose nothing.
 *   max_range cells, Chebyshev, 0 .. 32768; 0: unlimited.  A beam is traced for k <= max_range only: a cell further than max_range
 *             from the origin gets passes 0, low PWPP_VIEW_NO_HEIGHT and the base byte; every other cell gets exactly the unlimited
 *             values.  Beams from beyond the range still cross the cells inside it: no endpoint is dropped by range.
 *   occupancy (may be NULL) the base byte is occupancy_in[c], or PWPP_OCC_UNKNOWN when occupancy_in is NULL.  The output is
 *             PWPP_OCC_FREE iff the base byte equals PWPP_OCC_UNKNOWN, and passes[c] >= min_pass (compared unsigned), and `target` is
 *             NULL or target[c] != PWPP_VIEW_NO_HEIGHT and (int64)low[c] - (int64)target[c] <= clearance.  Everywhere else it is the
 *             base byte verbatim, whatever its value.  THEOREMS: the FREE cells of the input are a subset of the FREE cells of the
 *             output; no OCCUPIED or FREE byte of the input is changed.  occupancy == occupancy_in is allowed: the update in place.
 *   THE PRICE The beam is drawn from cell to cell, not from point to point: a crossed cell can lie up to one cell away from the true
 *             ray, and a single beam that grazes a wall's corner clears a cell the ray never entered.  min_pass >= 2 is the remedy:
 *             two endpoint hits must agree.  `clearance` bounds how high above the ground (target) the lowest beam may have passed:
 *             a beam three metres up says nothing about a bollard below it.
 *   beam_ground   enqueues, on the handle's stream: pwpp_rasterize_beams(g with flags 0, which); the ground raster of
 *             pwpp_rasterize_ground on the same grid (g->flags 0 or PWPP_GRID_GROUND_ONLY), quantised on the device by
 *             pwpp_viewshed_units -- this is `target`; and pwpp_beam_grid.  The origins {x, y, z} in metres become {ox, oy, eye} as
 *             pwpp_viewshed_obstacles turns them; clearance is in metres, finite and >= 0, through pwpp_viewshed_units.  occupancy_in
 *             is the caller's (may be NULL); in PWPP_MEM_DEVICE typically the bytes pwpp_viewshed_obstacles just wrote.  hits and
 *             zmin are returned where asked for, kept in the buffer otherwise.  The images are exactly what the three calls give one
 *             after the other.
 *   mem       PWPP_MEM_HOST stages every image through the handle's cluster buffer (pwpp_rasterize_beams: the ground-query staging
 *             buffer), synchronous; PWPP_MEM_DEVICE: device memory, the int32 images 4-byte aligned and no more, the bytes byte
 *             aligned, enqueued on the handle's stream.  PWPP_MEM_HOST_PINNED: PWPP_E_ARG.
 *   errors    pwpp_beam_grid: PWPP_E_ARG, named before the device is touched, in this order: a null handle, hits, zmin, origin, passes
 *             or low; nx, ny or frames < 1; nx or ny > 32768; nx * ny * frames beyond 2^31; max_range outside 0 .. 32768; min_pass <
 *             1; clearance < 0; the number of origins; an origin outside the image; an eye outside +-2^30, naming the entry; arrays
 *             that overlap (other than occupancy == occupancy_in); mem; in PWPP_MEM_DEVICE an int32 array below 4-byte alignment.
 *             pwpp_beam_ground: a null handle, grid, origin, passes or low; the flags; `which`; the grid's geometry and sides; a
 *             clearance that is not finite or negative; then as above from max_range to the overlaps, an origin that is not finite (z
 *             included) or outside the grid; then what pwpp_rasterize_obstacles rejects of the frame range and mem; the alignment;
 *             PWPP_E_STATE before any estimate call.
 *   buffers   The origins where there is one per frame, in PWPP_MEM_HOST the staged images and in the chained call its intermediate
 *             images lie in the cluster buffer: counted by pwpp_get_workspace_bytes, freed by pwpp_trim_workspace.
 * pwpp_fuse_obstacles, pwpp_match_obstacles, pwpp_costmap_obstacles and pwpp_evidence_obstacles do not consume these bytes by
 * themselves; feed them to pwpp_fuse_grid, pwpp_match_grid, pwpp_costmap_grid and pwpp_evidence_grid.  The same
 * bytes for every mem, alignment and value of the option "beams_path".  With none of the functions called nothing is allocated or
 * launched, and no result, state or timing of any other call changes. */
#define PWPP_HAS_BEAMS 1
#define PWPP_BEAMS_GROUND 1      /* `which`: the ground list */
#define PWPP_BEAMS_NONGROUND 2   /* `which`: the non-ground list (with the points the reflected-noise removal rejected) */

/* the endpoints of the beams of frames of the LAST estimate call -- like pwpp_rasterize_ground_returns */
PWPP_API int pwpp_rasterize_beams(pwpp_handle *h, const pwpp_ground_grid *g, int which, int frame_first, int frames, int mem,
                                  int32_t *hits /* [frames][ny][nx] */, int32_t *zmin /* same shape */);
/* any images: needs a handle (stream, buffer), no estimate call -- like pwpp_viewshed_grid */
PWPP_API int pwpp_beam_grid(pwpp_handle *h, int nx, int ny, int frames, int mem,
                            const int32_t *hits /* [frames][ny][nx] */, const int32_t *zmin /* same shape */,
                            const int32_t *target /* same shape, may be NULL */, const int8_t *occupancy_in /* same shape, may be NULL */,
                            const int32_t *origin /* HOST memory, n_origins x {ox, oy, eye} */, int n_origins,
                            int max_range /* cells, Chebyshev; 0: unlimited */, int min_pass, int clearance /* units, >= 0 */,
                            int32_t *passes /* [frames][ny][nx] */, int32_t *low /* same shape */,
                            int8_t *occupancy /* same shape, may be NULL, may be occupancy_in */);
/* endpoints + ground raster + beams for frames of the LAST estimate call, one call -- like pwpp_viewshed_obstacles */
PWPP_API int pwpp_beam_ground(pwpp_handle *h, const pwpp_ground_grid *g, int which,
                              const double *origin_xyz /* HOST, n_origins x {x, y, z} metres */, int n_origins,
                              int max_range, int min_pass, double clearance /* metres, >= 0 */, int frame_first, int frames, int mem,
                              const int8_t *occupancy_in /* may be NULL */, int32_t *passes, int32_t *low,
                              int8_t *occupancy /* may be NULL, may be occupancy_in */,
                              int32_t *hits /* may be NULL: kept */, int32_t *zmin /* may be NULL: kept */);
PWPP_API int32_t pwpp_beam_height(int32_t eye, int32_t z, int k, int n);   /* host only: the height of a beam at a crossed cell */

/* ---- a per-frame affine transform of the input, applied while binning (pwpp_set_input_transforms) ----------------------------
 * The pipeline assumes what the reference assumes: a levelled frame centred on the sensor, z up, the ground near -sensor_height.
 * A tilted or rolled mount, several sensors in their own frames, a driver that delivers millimetres, a cloud levelled by the IMU
 * every frame: instead of writing a transformed copy of each cloud first (one more read and one more write of the whole batch, and
 * the end of the in-place input paths), hand over T_f = [R | t], a 3 x 4 row-major float matrix per frame.
 *   Rule      With transforms set, every result of an estimate call is what the same call returns for the cloud whose points are
 *             T_f(p) -- bit for bit, in every layout, memory kind, mode, schedule and output option.  The kernels apply T_f where
 *             they read an input coordinate (no extra kernel, no extra bytes: nine multiplies and nine adds per point).
 *   T_f       Any affine map: rotation, scale, mirror.  Nothing checks orthonormality.  The arithmetic is part of the contract
 *             (no FMA is formed anywhere):
 *                 x' = fl32(fl32(fl32(fl32(r00 * x) + fl32(r01 * y)) + fl32(r02 * z)) + t0)     y', z' alike with rows 1 and 2
 *             so the identity matrix is NOT "off": it turns -0.0 into +0.0 (-0.0 + 0.0 is +0.0) and leaves every other value alone.
 *             The fourth column of the input (intensity) passes through untouched.  Non-finite coordinates give what IEEE gives:
 *             0 * inf is NaN, so ONE infinite coordinate of a point poisons all three: an output is NaN where the matrix has a zero
 *             in that coordinate's column and +-inf or NaN elsewhere -- also under the identity, which returns {inf, NaN, NaN}
 *             for {inf, y, z}.  A NaN coordinate makes NaN of all three.
 *   Tests     All tests of the reference act on the transformed values: RNR's vertical angle and z guard, the range test, and the
 *             skip marker z == FLT_MIN.  An input z of FLT_MIN is not special unless it maps to FLT_MIN; a point that maps onto
 *             FLT_MIN exactly is skipped.
 *   Setting   `T` is count x 12 floats in HOST memory, copied at the call; sticky; applies to the estimate calls launched
 *             afterwards.  count == 1: that transform for every frame of every later call.  count > 1: entry i is for frame i (in
 *             PWPP_MODE_STREAMS: stream i) and count must equal `frames` of each later call -- an estimate call with another
 *             number of frames returns PWPP_E_ARG and launches nothing (the results of the call before stay readable).
 *             T == NULL or count == 0 turns it off: nothing is allocated or launched for it, results are byte-identical to a
 *             handle that never had transforms.  PWPP_E_ARG: a negative count, more than 65535 entries, an entry that is not
 *             finite.  A pipe's handles take the setting through pwpp_pipe_handle, like the other settings.
 *   Getters   pwpp_get_ground_xyz / pwpp_get_nonground_xyz (getGround() / getNonground()) return TRANSFORMED coordinates: the rows
 *             of the cloud the rule speaks of.  pwpp_get_*_records, pwpp_get_all_records and the device records stay verbatim
 *             copies of the input bytes, in the SENSOR's frame ("bytes are copied, never interpreted" keeps holding).  Point
 *             distances, centers, normals, patch records, the adaptive state, pwpp_query_ground and pwpp_rasterize_ground live
 *             in the transformed frame: carry query positions there with pwpp_transform_points.
 * pwpp_transform_points: host only, no device needed.  out[i] = T(xyz[i]) for m rows of {x, y, z}, by the formula above, compiled
 * from the same function the kernels use -- for query positions, detection boxes or a second sensor's returns that must land in
 * the model's frame with exactly this library's rounding.  out may be xyz itself.  m == 0 is PWPP_OK. */
#define PWPP_HAS_INPUT_TRANSFORM 1
PWPP_API int pwpp_set_input_transforms(pwpp_handle *h, const float *T /* count x 12, host memory */, int count);
PWPP_API int pwpp_transform_points(const float T[12], const float *xyz /* (m,3) row-major */, int64_t m, float *out /* (m,3) */);

/* Overlap mode (ON by default): batches of 128 frames or more are processed as two frame ranges -- binning
 * and index lists of both on the handle's main stream, each range's plane fits on a stream of its own -- so
 * that the stages of one range fill the wave slots the other leaves empty (binning and index lists are bound
 * by memory, the plane fits by their dependent chains).  Same results; per-kernel profiling (pwpp_set_profiling) and PWPP_ORDER_REFERENCE use the single-stream
 * schedule.  pwpp_set_overlap(h, 0) / PWPP_OVERLAP=0 select that schedule for everything. */
PWPP_API int pwpp_set_overlap(pwpp_handle *h, int on);
/* one-pass binning (fixed bin segments): batches launched that way and how many of
 * them had at least one frame redone on the exact two-pass path because a bin outgrew its segment.  Finishes the
 * batch in flight first.  No reference counterpart (its bins are unbounded vectors, patchworkpp.cpp:578-622). */
PWPP_API int pwpp_get_one_pass_stats(pwpp_handle *h, int64_t *batches, int64_t *redone);
/* ... and the same per FRAME: frames that went through one-pass binning, and how many of them were redone.  An
 * overflow costs the frames it happened in, not their batch (round 5): such a frame is binned again, exactly and
 * in place, while the other frames' results stand; only a frame too large for its own slots of the one-pass layout
 * (or the option "redo_whole_batch") sends the whole batch through the two-pass path, and then every frame counts. */
PWPP_API int pwpp_get_redo_stats(pwpp_handle *h, int64_t *frames_one_pass, int64_t *frames_redone);
/* ... and what keeps that rare (round 6): a part's segment holds ~1.06 x the largest count the part has had, and every frame owns an
 * OVERFLOW ARENA behind its segments -- a part that outgrows its segment is moved there as a whole by the scan kernel, on the device
 * (the cost of copying that part), and only a frame whose arena runs out goes back to the host.  frames_with_moved_parts counts the
 * frames that took that path; slots_per_frame / arena_slots describe the current table (0 before the first one-pass batch). */
PWPP_API int pwpp_get_arena_stats(pwpp_handle *h, int64_t *frames_with_moved_parts, int64_t *slots_per_frame, int64_t *arena_slots);


/* ---- batches in flight (no reference counterpart; round 5) --------------------------------------------------------------------
 * A pipe keeps `depth` batches of independent frames enqueued: it owns `depth` handles (each with its own workspace and HIP streams,
 * each on the single-stream schedule) and deals the submitted batches to them in turn.  pwpp_pipe_submit waits for the batch the
 * next handle launched `depth` submits ago (its results are complete then, and are replaced by the new batch), launches the new one
 * and returns that handle: the caller reads the results through the usual getters after pwpp_synchronize(handle), any time before
 * the handle comes round again.  The ramp-up of one batch (binning, nothing to overlap with) then runs under the ramp-down of
 * the one before (last plane fits, index lists): 2.32-2.46 instead of 2.49-2.63 ms per 1024-frame batch with depth 2
 * (profiles/r05_pipelined_batches.txt; depth 3: +0.5 %).  `mem` as in pwpp_estimate_ground_batch (PWPP_MEM_DEVICE or
 * PWPP_MEM_HOST_PINNED to stay asynchronous), `mode` likewise: PWPP_MODE_FRESH, or PWPP_MODE_STREAMS (round 6) for stateful streams
 * in disjoint GROUPS -- a stream's frames must stay in order on ONE handle, so handle g owns the streams of group g
 * (pwpp_pipe_set_num_streams sizes every handle's group) and the caller submits the groups round robin: submit k carries the next
 * frames of group k mod depth (reference use: demo_sequential.cpp:54-67, one long-lived object per stream).  depth 1..4.
 * The handles belong to the pipe: a pointer from pwpp_pipe_handle / pwpp_pipe_submit is INVALID after pwpp_pipe_destroy. */
typedef struct pwpp_pipe pwpp_pipe;
PWPP_API int pwpp_pipe_create(const pwpp_params *p, int device, int depth, pwpp_pipe **out);
PWPP_API int pwpp_pipe_submit(pwpp_pipe *pipe, const float *const *points, const int32_t *n, int frames, int cols, int layout, int mem,
                              int mode, pwpp_handle **holder);
/* pwpp_set_num_streams(streams_per_handle) on every handle of the pipe: `depth` groups of that many fresh streams */
PWPP_API int pwpp_pipe_set_num_streams(pwpp_pipe *pipe, int streams_per_handle);
/* waits for every batch in flight */
PWPP_API int pwpp_pipe_drain(pwpp_pipe *pipe);
/* the pipe's handles (options, statistics, getters): index 0 .. depth - 1; NULL beyond */
PWPP_API pwpp_handle *pwpp_pipe_handle(pwpp_pipe *pipe, int index);
PWPP_API int pwpp_pipe_destroy(pwpp_pipe *pipe);

/* Tuning and test switches (no reference counterpart).  The environment variables PWPP_DEBUG_FLAGS,
 * PWPP_FIT_PLAN, PWPP_NO_ONE_PASS, PWPP_ONE_PASS_MIN_FRAMES, PWPP_ONE_PASS_SCALE, PWPP_OVERLAP,
 * PWPP_OVERLAP_RANGES, PWPP_FIT_STREAMS, PWPP_HI_SPLIT, PWPP_HI_SPLIT_ZONES and PWPP_EXACT_MOMENTS set the same options ONCE, in pwpp_create (which says so on stderr); nothing reads the
 * environment afterwards.  None of them changes a result, except the one that says so:
 *   "exact_moments"       "1" (default): the plane-fit sums of 4+ points exact on the reference's floats (2^-30 m grid, contract v4);
 *                         "0": rounds 3-5's 2^-21 m grid -- 7 % faster, off the reference by a few indices on 0.2 % of varied frames
 *                         (see pwpp_get_ground_indices above).  May be changed between calls.
 *   "split_k5"            "1" (default): calls with up to 64 stateful streams run K5 (GLE / TGR / thresholds) in two launches -- the index lists
 *                         wait for the first only; the statistics over the streams' A-GLE histories (two chains of ~1000 dependent f64 adds
 *                         in the reference's order) run on the handle's second stream, under K6 and the host's turn-around: one stream in steady
 *                         state 108 -> 100 us per frame.  "2": the second launch starts only when the lists are written (not beside K6): the
 *                         lists another ~4-5 us earlier, the state ~15 us later (a caller that steps the stream again at once waits for it there).  "0": one kernel
 *   "fit_plan"            which fit kernel handles which patch sizes, e.g. "W16:1023,W64.2:65535"; "" = automatic
 *   "one_pass"            "0": always the two-pass binning
 *   "redo_whole_batch"    "1": a segment overflow of the one-pass binning redoes every frame of the batch (rounds 1-4) instead of
 *                         the frames that overflowed
 *   "one_pass_min_frames" smallest batch that takes the one-pass binning (default 1; rounds 1-3: 5 for stream batches, whose state
 *                         must be copied aside for a redo -- the binning pipeline now copies it itself, off the chain)
 *   "one_pass_scale"      scales the head-room of the one-pass segments (default 4 = 1.0625 x the largest count seen + 2 sqrt + 16 slots; tests
 *                         use small values to force overflows: first the arena, then the host's redo)
 *   "overlap_ranges"      frame ranges of the overlap mode (default 2; more were slower: 3.38 ms vs 2.86 ms with 4)
 *   "fit_streams"         streams the ranges' fit stages are dealt to (1..8, default 2): binning and lists of the overlap
 *                         mode run on the main stream
 *   "hi_split"            metres above the ground level (-sensor_height) where the "high" part of a bin begins
 *                         (default 0.6; 1e30 = no high parts): the fit passes skip a high part whenever they can
 *                         prove that none of its points can enter the pass
 *   "hi_split_zones"      how many zones' bins are stored in two parts (0..4, default 1: the near zone)
 *   "records_path"        how the point records are gathered (pwpp_set_point_records): "0" (default) the kernel chooses by row size and
 *                         alignment; "1": one lane per row at every size (the yardstick of tools/point_records_cost.py); "2": never
 *                         the 16-byte pieces (tests)
 *   "clusters_path"       how the obstacle clusters are labelled (pwpp_label_grid, pwpp_label_obstacles): "0" (default) tiles of
 *                         64 x 16 cells in LDS, then the tiles' borders; "1": one global union-find without LDS (the yardstick of
 *                         tools/obstacle_clusters_cost.py).  The results are identical bytes.
 *   "boxes_path"          how the points reach the rows of the obstacle boxes (pwpp_box_obstacles): "0" (default) the faster of the
 *                         two by tools/obstacle_boxes_cost.py; "1": every counted lane issues its atomics on its row (the yardstick);
 *                         "2": the lanes of a wave that name the same row are summed first, one set of atomics per distinct row.
 *                         The results are identical bytes.
 *   "hulls_path"          how a row's hull and rectangle are computed from its candidates (pwpp_hull_obstacles): "1": a lane per row,
 *                         serial gift wrapping, then every edge's rectangle in turn (the yardstick); "2": a wave per row -- a march
 *                         step is one strided sweep by 64 lanes and a butterfly under the march's total order, the hull lies in
 *                         LDS, the edges are dealt to the lanes; "0" (default): what tools/obstacle_hulls_cost.py decided.  The
 *                         same bytes for every value.
 *   "distance_path"       how the column pass of the obstacle distances runs (pwpp_distance_grid, pwpp_distance_obstacles): "0"
 *                         (default) the strip's rows in LDS where they fit, outward from the cell's own row with the exact early
 *                         exit; "1": every row from global memory, no LDS, no early exit (the yardstick of
 *                         tools/obstacle_distance_cost.py).  The results are identical bytes.
 *   "visibility_path"     how the line-of-sight free space tests a cell (pwpp_visibility_grid, pwpp_visibility_obstacles): "0"
 *                         (default) a bit image of the frame, one ballot per 64 cells, kept in LDS where it fits; "1": no bit
 *                         image, no LDS, every test reads count in global memory (the yardstick of
 *                         tools/obstacle_visibility_cost.py).  The results are identical bytes.
 *   "fusion_path"         how the occupancy fusion forms a sample's cell (pwpp_fuse_grid, pwpp_fuse_obstacles): "0" (default)
 *                         u = (fx - x0) * (1 / cell) where the frame images' cell size is a power of two -- the reciprocal is
 *                         exact and the product the same bits as the quotient -- and the division otherwise; "1": always the
 *                         double division as the contract writes it (the yardstick of tools/occupancy_fusion_cost.py).  The
 *                         results are identical bytes.
 *   "elevation_path"      how the elevation fusion divides (pwpp_fuse_height_grid, pwpp_fuse_ground): "1": the quotients u, v and the share
 *                         a capped mean forgets by divisions as the contract writes them (the yardstick); "2": the product with the exact
 *                         reciprocal where the frame images' cell size is a power of two, and an exact multiply-shift by n_max; "0"
 *                         (default): what tools/elevation_fusion_cost.py decided.  The same bytes for every value.
 *   "terrain_path"        how the terrain analysis sums a window (pwpp_terrain_grid, pwpp_terrain_ground): "1": every lane walks its whole
 *                         window in LDS (the yardstick); "2": separable, the sums of every row over dx first, then 2r+1 rows combined with
 *                         their dy; "0" (default): per radius what tools/terrain_cost.py decided.  The same bytes for every value.
 *   "reach_path"          how the cost-to-reach field is relaxed (pwpp_reach_grid, pwpp_reach_ground), a workgroup per frame either way:
 *                         "1": sweeps over the frame's cells in global memory until a sweep changes nothing (the yardstick); "2": the
 *                         frame's tiles of 32 x 32 cells, each relaxed in LDS with a halo of one cell, a tile revisited when a
 *                         neighbour's border changed; "0" (default): what tools/reach_cost.py decided.  The same bytes for every value.
 *   "route_path"          how the routes are dealt (pwpp_route_grid, pwpp_plan_grid): "1": a lane per route, wholly serial, the waypoints by
 *                         a second walk through from (the yardstick); "2": a wave per route -- every lane takes the hops, the route's
 *                         last 512 cells lie in LDS, the shortcut candidates go to the lanes from the far end and a ballot picks the
 *                         largest clear one; "0" (default): what tools/route_cost.py decided.  The same bytes for every value.
 *   "footprint_path"      how the footprints are dealt (pwpp_footprint_grid): "1": a lane per pose, serial over its window, then a lane per
 *                         trajectory over the pose rows (the yardstick); "2": a wave per trajectory -- its steps fill the wave's lanes
 *                         first, the cells of a pose's window are dealt to the lanes the steps leave over, the folds cross the
 *                         lanes by shuffles and the trajectory's summary stays in registers; "0" (default): what
 *                         tools/footprint_cost.py decided -- "2" for a call whose max(front, rear) + half_width is 504 ticks or more
 *                         and that asks for no pose rows (it stops a trajectory at its first hit) or reads dist2, "1" otherwise.
 *                         The same bytes for every value.
 *   "viewshed_path"       how the viewshed tests a cell (pwpp_viewshed_grid, pwpp_viewshed_obstacles), a lane per cell either way: "1":
 *                         every test reads count and every rise reads block in global memory (the yardstick); "2": the occupancy packed
 *                         into the visibility's bit image, the rows a run of 256 cells can touch kept in LDS where the frame's image
 *                         fits 128 KiB, a rise fetched from global memory only where a bit is set; "0" (default): what
 *                         tools/viewshed_cost.py decided -- "2" for a call with max_range 0, "1" under a max_range.  The same bytes
 *                         for every value.
 *   "costmap_path"        how the costmap's fold is dealt (pwpp_costmap_grid, pwpp_costmap_obstacles): "1": a lane per cell, the inflation
 *                         curve read from global memory (the yardstick); "2": the curve staged once per workgroup into LDS, four
 *                         consecutive cells a lane, the byte images as one dword where their address allows; "0" (default): what
 *                         tools/costmap_cost.py decided -- "2" for a call of 2^24 cells or more, "1" below.  The same bytes for every value.
 *   "match_path"          how the scan match reads the map (pwpp_match_grid, pwpp_match_obstacles): "1": every map read comes from
 *                         global memory (the yardstick of tools/scan_match_cost.py); "2": the rectangle of the map that the
 *                         landings of a (frame, candidate) reach under the window is copied into LDS once per workgroup where it
 *                         holds at most 65536 cells, and read from global memory where it does not; "0" (default): whichever of
 *                         the two that tool found faster.  The results are identical bytes.
 *   "evidence_path"       where the map evidence sums a row's counters (pwpp_evidence_grid, pwpp_evidence_obstacles): "1": in the output
 *                         rows, with global atomics (the yardstick of tools/evidence_cost.py); "2": a workgroup sums a run of 2048
 *                         cells in a table in LDS first where max_rows <= PWPP_EVID_LDS_ROWS, and as "1" where it is not; "0"
 *                         (default): whichever of the two that tool found faster on 256 x 256 cells.  The results
 *                         are identical bytes.
 *   "debug_flags"         4: timing probes of the fit chain; 8: timing probes of the binning, scan and GLE kernels;
 *                         16: exact binning arithmetic only;
 *                         128: the first pass of the history statistics always as the reference's sequential sum (no exact shortcut);
 *                         64: before a call that skips the clearing kernel (the last call's K5 zeroed this call's counters),
 *                         read the counters back and fail with PWPP_E_STATE unless every word is zero;
 *                         2048: no overflow arena (a full segment sends its frame back to the host, as in rounds 2-5);
 *                         16384 / 32768: force the fall-back paths of the lowest-point selection
 * Returns PWPP_E_ARG for an unknown name or a value out of range. */
PWPP_API int pwpp_set_option(pwpp_handle *h, const char *name, const char *value);
/* The 64 timing probes of the last call when "debug_flags" has bit 2 set (device-side timestamps along the fit chain of the
 * largest patch, (code << 56) | 100 MHz ticks; slots 60-62: first start, last end, the patch's size): what tools/brows_chain.py
 * prints.  PWPP_E_STATE if no call has run.  A measurement aid; results never depend on it. */
PWPP_API int pwpp_debug_read(pwpp_handle *h, unsigned long long *out64);
/* Frees everything whose size follows the batch (a handle that processed one large batch otherwise keeps it, e.g. 9.7 GB
 * after 1024 KITTI frames with one-pass binning): inputs staged from the host, the bin-ordered planes, the index lists,
 * every per-frame table and patch record, the state of PWPP_MODE_FRESH frames and the one-pass snapshots.  Kept: the
 * streams' state (thresholds, histories, plane members) and the per-handle tables (a few KB).  The results of the last
 * call are gone: fetch them first.  The next call allocates again. */
PWPP_API int pwpp_trim_workspace(pwpp_handle *h);
/* device memory the handle holds right now, in bytes: EVERY device allocation of the handle (inputs handed over as device
 * buffers are the caller's); after pwpp_trim_workspace what is left is the streams' state and the per-handle tables */
PWPP_API int64_t pwpp_get_workspace_bytes(pwpp_handle *h);

#ifdef __cplusplus
}
#endif
#endif /* PWPP_H */
