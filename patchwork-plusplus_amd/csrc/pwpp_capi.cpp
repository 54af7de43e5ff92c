// pwpp_capi.cpp -- host side of libpwpp_hip.so: the C-ABI of include/pwpp.h.
//
// Owns the device workspace, the per-stream adaptive state and the HIP stream of a handle,
// validates parameters exactly where the reference constructor would read them
// (/root/reference/cpp/patchworkpp/include/patchwork/patchworkpp.h:120-150) and drives the six
// kernels of pwpp_kernels.hip.  There is no CPU fallback: without a GPU every compute entry
// point fails with PWPP_E_NODEVICE / PWPP_E_HIP.
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <string>
#include <new>
#include <utility>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/pwpp.h"
#include "pwpp_boxes.h"
#include "pwpp_hull.h"
#include "pwpp_dev.h"
#include "pwpp_distance.h"
#include "pwpp_elevation.h"
#include "pwpp_evidence.h"
#include "pwpp_fusion.h"
#include "pwpp_match.h"
#include "pwpp_costmap.h"
#include "pwpp_reach.h"
#include "pwpp_route.h"
#include "pwpp_footprint.h"
#include "pwpp_terrain.h"
#include "pwpp_tracks.h"
#include "pwpp_viewshed.h"
#include "pwpp_beams.h"
#include "pwpp_visibility.h"

static_assert(sizeof(pwpp_state) == sizeof(PwppStateScalar), "pwpp_state must mirror PwppStateScalar");
static_assert(sizeof(pwpp_ground_sample) == sizeof(PwppGroundSample) && sizeof(pwpp_ground_sample) == 16, "pwpp_ground_sample must mirror PwppGroundSample");
static_assert(sizeof(pwpp_ground_grid) == sizeof(PwppGroundGrid) && sizeof(pwpp_ground_grid) == 40, "pwpp_ground_grid must mirror PwppGroundGrid");

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return fail(PWPP_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// The handle's workspace: every buffer is declared ONCE, with its lifetime, and enrols itself in the list it is given
// (pwpp_handle::bufs).  pwpp_destroy, pwpp_trim_workspace and pwpp_get_workspace_bytes are loops over that list.
enum Lifetime {
    kPerBatch,   // its size follows the batch: pwpp_trim_workspace frees it
    kPerHandle,  // stays until pwpp_destroy
};

struct BufBase {
    const bool on_device, per_batch;
    virtual size_t bytes() const = 0;
    virtual void release() = 0;
    BufBase(const BufBase &) = delete;
    BufBase &operator=(const BufBase &) = delete;

  protected:
    BufBase(std::vector<BufBase *> &list, bool on_device_, Lifetime life) : on_device(on_device_), per_batch(life == kPerBatch) { list.push_back(this); }
    ~BufBase() = default;
};

template <class T>
struct DevBuf final : BufBase {
    T *p = nullptr;
    size_t cap = 0;  // elements
    DevBuf(std::vector<BufBase *> &list, Lifetime life) : BufBase(list, true, life) {}
    size_t bytes() const override { return cap * sizeof(T); }
    void swap(DevBuf &o) {
        std::swap(p, o.p);
        std::swap(cap, o.cap);
    }
    int ensure(size_t n) {
        if (n <= cap) return PWPP_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        // (head-room so that sizes creeping up do not reallocate every call: an eighth, at most 4 M elements -- an eighth of the
        // bin-ordered planes of a 1024-frame batch was 0.7 GB of nothing)
        const size_t want = n + (n / 8 < ((size_t)4 << 20) ? n / 8 : ((size_t)4 << 20)) + 64;
        hipError_t e = hipMalloc((void **)&p, want * sizeof(T));
        if (e != hipSuccess) return fail(PWPP_E_NOMEM, "hipMalloc(%zu bytes) failed: %s", want * sizeof(T), hipGetErrorString(e));
        cap = want;
        return PWPP_OK;
    }
    void release() override {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

template <class T>
struct PinnedBuf final : BufBase {
    T *p = nullptr;
    size_t cap = 0;
    PinnedBuf(std::vector<BufBase *> &list, Lifetime life) : BufBase(list, false, life) {}
    size_t bytes() const override { return cap * sizeof(T); }
    int ensure(size_t n) {
        if (n <= cap) return PWPP_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = n + n / 8 + 64;
        hipError_t e = hipHostMalloc((void **)&p, want * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) return fail(PWPP_E_NOMEM, "hipHostMalloc(%zu bytes) failed: %s", want * sizeof(T), hipGetErrorString(e));
        cap = want;
        return PWPP_OK;
    }
    void release() override {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

// the per-point outputs a call may write next to its index lists
enum Output { kLabels, kPointPlanes, kPointRecords };
const char *const kOutputMissing[] = {"the last call ran without labels (pwpp_set_labels, PWPP_ORDER_CLOUD)",
                                      "the last call ran without point planes (pwpp_set_point_planes)",
                                      "the last call ran without point records (pwpp_set_point_records)"};

// "The OTHER copy of the counters (d_parts / d_results) is clean": what the last call's K5 zeroed, and in which allocations.
struct CleanCopy {
    bool valid = false;
    int frames = 0, slabs = 0;  // for a call of this many frames and slabs (1: one-pass, 3: two-pass)
    const void *parts = nullptr, *results = nullptr;
    size_t parts_cap = 0, results_cap = 0;
    void capture(const pwpp_handle *h, int frames_, int slabs_);
    bool matches(const pwpp_handle *h, int frames_, int slabs_) const;
};

const char *kKernelNames[PWPP_NUM_KERNELS] = {"k_czm_bin", "k_czm_scan", "k_czm_scatter", "k_fit_w64<16,64>", "k_fit_w64<64,p>",
                                              "k_fit[2]", "k_fit[3]", "k_fit[4]", "k_fit_stream", "k_gle_tgr", "k_emit"};  // fit slots: the classes of the big-batch plan (p = 4 big bins per wave on scans of KITTI density, 2 on denser ones)

std::atomic<bool> g_slot0_one_pass{false};  // diagnostic only (pwpp_kernel_name); handles on different threads may race to set it

}  // namespace

struct pwpp_handle {
    std::vector<BufBase *> bufs;  // every DevBuf / PinnedBuf below, in declaration order (declared first: the buffers enrol as they are built)
    pwpp_params params;
    PwppDevParams dp;
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t aux_stream = nullptr;  // second stream for the latency plan (few frames)
    hipEvent_t aux_fork = nullptr, aux_join = nullptr;
    bool k5_tail_unjoined = false;  // the last call left K5's second part on aux_stream (aux_join recorded behind it): the main stream has not waited for it yet
    bool k5_tail_unsynced = false;  // ... and neither has the host
    bool hist_check_due = false;    // the fill of the streams' histories after the last call has not been looked at yet (settle_k5_tail)
    int split_k5 = 1;               // option "split_k5": a few stateful streams run K5 in two launches (k_gle_tgr PART 1 / 2)
    bool overlap = true;   // pwpp_set_overlap: big batches as a pipeline of frame ranges over the two streams (default on)
    int overlap_ranges = 2;  // (more ranges were slower at every setting tried: each range's fit kernels end with the tail of their
                             // longest waves -- docs/history/design_through_round4.md section 9)
    std::vector<hipEvent_t> ev_ranges;  // two per frame range: binned, fitted
    int num_fit_streams = 2;            // option "fit_streams": streams the ranges' fit stages are dealt to (aux_stream + extra_streams)
    std::vector<hipStream_t> extra_streams;
    // tuning / test options (pwpp_set_option; the PWPP_* environment variables are read ONCE, in pwpp_create)
    int debug_flags = 0;
    std::string fit_plan;
    bool no_one_pass = false;
    int one_pass_min_frames = 1;     // stream batches (round 4: the state a redo starts from is copied by extra workgroups of k_czm_scan, no
                                     // copy commands in front of the pipeline any more: one stream 112.8 -> 106.9 us of GPU time, 139 -> 131 us per call)
    int one_pass_min_fresh = 1;      // ... and batches of FRESH frames (a single frame: 118 -> 107 us in round 3)
    double one_pass_scale = 4.0;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    hipEvent_t ev_k[PWPP_NUM_KERNELS + 1] = {};
    bool profiling = false;
    bool profile_pending = false;
    double prof_ms[PWPP_NUM_KERNELS] = {};
    int64_t prof_launches[PWPP_NUM_KERNELS] = {};

    // last call
    int frames = 0;
    int mode = PWPP_MODE_FRESH;
    bool have_results = false;
    bool pending = false;  // launches in flight, results not yet fetched
    double time_us = 0.0;
    std::vector<PwppFrameDesc> descs;  // host copy of the last batch (device pointers inside)
    std::vector<PwppFrameDesc> descs_on_device;  // what d_frames holds
    const PwppFrameDesc *descs_dev_ptr = nullptr;
    // one-pass binning (fixed bin segments, DESIGN.md section 3 K1'): state of the batch in flight
    bool one_pass = false;           // the batch in flight uses fixed segments; overflow flags are checked when it lands
    int one_pass_holdoff = 0;        // batches to run on the two-pass path after an overflow
    int64_t slots_per_frame = 0;     // of the current capacity table: the parts' segments + the frame's overflow arena
    uint32_t arena_base = 0, arena_slots = 0, arena_spill = 0;  // the arena of the current table (pwpp_dev.h): first slot, slots (0: none), room for spilled records
    DevBuf<uint2> d_arena_tag{bufs, kPerBatch};  // [frames][arena_spill]
    int cap_max_n = -1;              // largest frame the capacity table on the device was built for
    bool cap_few = false;            // ... and whether it was built with the head-room of calls of a few frames
    int max_n = 0;
    int64_t total_points = 0;
    int cols = 4, layout = 0;
    long long one_pass_batches = 0, one_pass_redone = 0;  // batches on the one-pass path; of those, batches with at least one frame redone
    long long one_pass_frames = 0, one_pass_redone_frames = 0;  // the same per frame (pwpp_get_redo_stats)
    std::vector<uint8_t> frame_two_pass;  // frames of the last one-pass batch that were redone in place (compact layout at their own first slot)
    bool redo_whole_batch = false;        // option "redo_whole_batch": an overflow redoes every frame of the batch (rounds 1-4; tests, A/B)
    long long fixed_up_frames = 0;   // frames finished by k_fit_fixup (a patch needed the plane fitted before it)
    long long arena_frames = 0;      // frames in which k_czm_scan moved overgrown parts into the overflow arena (PwppFrameResult.overflow bit 3)
    long long clamped_frames = 0;    // frames with a patch whose final ground set spanned more than z0 +- ZR (PwppFrameResult.overflow bit 2)

    // workspace
    DevBuf<PwppFrameDesc> d_frames{bufs, kPerBatch};
    PinnedBuf<PwppFrameDesc> h_frames{bufs, kPerHandle};
    PinnedBuf<int64_t> h_base{bufs, kPerHandle};
    DevBuf<float> d_in{bufs, kPerBatch};  // staging for host inputs
    DevBuf<uint16_t> d_codes{bufs, kPerBatch};
    DevBuf<float> d_sorted_z{bufs, kPerBatch};  // the bin-ordered planes (pwpp_dev.h): z, {x, y}, cloud index
    DevBuf<float2> d_sorted_xy{bufs, kPerBatch};
    DevBuf<int> d_sorted_idx{bufs, kPerBatch};
    DevBuf<float2> d_bin_origin{bufs, kPerHandle};  // [B] origins of the fixed-point plane-fit sums
    DevBuf<float4> d_bin_bbox{bufs, kPerHandle};  // [B] {xmin, xmax, ymin, ymax} of every bin (the fit kernels' skip test of the high parts)
    DevBuf<uint8_t> d_member{bufs, kPerBatch};  // membership plane (pwpp_dev.h, PWPP_SLOT_ALIGN): one bit per slot + PWPP_MEMBER_PAD bytes per part
    DevBuf<int32_t> d_out{bufs, kPerBatch};
    DevBuf<unsigned long long> d_ord_a{bufs, kPerBatch}, d_ord_b{bufs, kPerBatch};  // scratch of the reference-order mode (long sub-lists)
    DevBuf<uint32_t> d_ord_work{bufs, kPerBatch};  // ... and its work lists: the sub-lists above 256 entries of every frame
    int output_order = PWPP_ORDER_SCATTER;
    unsigned outputs = 0;           // bits 1 << Output: what the next call writes (pwpp_set_labels, pwpp_set_point_planes, pwpp_set_point_records)
    unsigned outputs_last = 0;      // ... and what the last call wrote (PWPP_ORDER_CLOUD implies the labels)
    DevBuf<uint8_t> d_labels{bufs, kPerBatch};  // [total points + 16] one PWPP_LABEL_* per point, laid out like d_out
    DevBuf<uint32_t> d_label_tiles{bufs, kPerBatch};  // PWPP_ORDER_CLOUD: [frames][tiles per frame] counts of the compaction (PwppBatch.label_tiles)
    DevBuf<int32_t> d_pt_patch{bufs, kPerBatch};  // [total points] the row of every point's patch (-1: none), laid out like d_out
    DevBuf<float> d_pt_dist{bufs, kPerBatch};  // [total points] its signed distance to that patch's plane (NaN: none)
    DevBuf<int32_t> d_pt_rows{bufs, kPerBatch};  // [frames][B] K9's bin -> row table (PwppBatch.pt_rows)
    std::vector<float> input_xf;    // pwpp_set_input_transforms: 12 floats per entry, copied at that call; empty = off.  One entry applies to
                                    // every frame, several to frame i each (estimate_batch points the frame descriptors at them)
    DevBuf<float> d_xf{bufs, kPerHandle};    // the transforms of the last call on the device (PwppFrameDesc.xf points into it); nothing before the first call with transforms
    PinnedBuf<float> h_xf{bufs, kPerHandle}; // ... and what it holds
    size_t xf_on_device = 0;                 // floats of h_xf that d_xf mirrors
    int record_bytes = 0;           // bytes per row of the last call's records (0: no call yet)
    int records_path = 0;           // option "records_path"
    DevBuf<uint8_t> d_records{bufs, kPerBatch};  // [total points][record_bytes] + 64: the records of the listed points, rows laid out like d_out
    // ground queries of the last call's results (pwpp_query_ground, pwpp_rasterize_ground): nothing is allocated before the first one
    DevBuf<int32_t> d_ground_rows{bufs, kPerBatch};   // [frames][B] bin -> row of the last call (PwppGroundView.rows)
    DevBuf<uint32_t> d_ground_stage{bufs, kPerBatch};  // PWPP_MEM_HOST queries: the sections of the call, in 4-byte words (Staging)
    // obstacle clusters (pwpp_label_grid, pwpp_label_obstacles): nothing is allocated before the first of them
    DevBuf<uint32_t> d_clusters{bufs, kPerBatch};  // the cluster buffer, in 4-byte words: the kernels' working image and chunk counts, then whatever
                                                   // images, table, counts and point ids the call stages or keeps (Staging)
    int clusters_path = 0;          // option "clusters_path": 0 = tiles in LDS, then their borders; 1 = the global union-find alone (yardstick)
    int distance_path = 0;          // option "distance_path": 0 = the strip's rows in LDS, outward with the early exit; 1 = global memory, every row (yardstick)
    int visibility_path = 0;        // option "visibility_path": 0 = the bit image, in LDS where it fits; 1 = count in global memory, no bit image (yardstick)
    int viewshed_path = 0;          // option "viewshed_path": 0 = what tools/viewshed_cost.py decided (pwpp_viewshed_path_of: 2 for an unlimited call, 1 under a max_range); 1 = count and block in global memory (yardstick); 2 = the bit image, in LDS where it fits, a rise fetched only where a bit is set
    int beams_path = 0;             // option "beams_path": 0 = what tools/beams_cost.py decided (pwpp_beams_path_of: 2, which won every configuration); 1 = a lane per endpoint cell, atomics on the global images after a fill (yardstick); 2 = a workgroup per tile of 64 x 64 cells, the tile's passes and low in LDS
    int fusion_path = 0;            // option "fusion_path": 0 = the product with 1 / cell where the cell size is a power of two; 1 = always the division (yardstick)
    int elevation_path = 0;         // option "elevation_path": 0 = what tools/elevation_fusion_cost.py decided; 1 = the divisions as written (yardstick); 2 = the reciprocal of a power-of-two cell and the multiply-shift for the capped mean
    int terrain_path = 0;           // option "terrain_path": 0 = per radius what tools/terrain_cost.py decided; 1 = every lane walks its whole window (yardstick); 2 = separable, row sums first
    int costmap_path = 0;           // option "costmap_path": 0 = what tools/costmap_cost.py decided (2 from PWPP_COSTMAP_QUADS_FROM_CELLS cells a call, 1 below); 1 = a lane per cell, the curve read from global memory (yardstick); 2 = the curve staged in LDS, four cells a lane
    int route_path = 0;             // option "route_path": 0 = what tools/route_cost.py decided; 1 = a lane per route, wholly serial (yardstick); 2 = a wave per route, the route's last cells in LDS, the shortcut candidates dealt to the lanes
    int footprint_path = 0;         // option "footprint_path": 0 = what tools/footprint_cost.py decided (2 under a large footprint for trajectory rows alone or with dist2, 1 otherwise); 1 = a lane per pose, then a lane per trajectory over the pose rows (yardstick); 2 = a wave per trajectory, small windows packed, the folds by shuffles
    int reach_path = 0;             // option "reach_path": 0 = what tools/reach_cost.py decided; 1 = sweeps over global memory, a workgroup per frame (yardstick); 2 = the frame's tiles relaxed in LDS, dirty tiles revisited
    int evidence_path = 0;          // option "evidence_path": 0 = what tools/evidence_cost.py decided; 1 = the sums go to the rows with global atomics (yardstick); 2 = a workgroup sums a run of cells in LDS first where the rows fit
    int match_path = 0;             // option "match_path": 0 = what tools/scan_match_cost.py decided; 1 = every map read from global memory (yardstick); 2 = the map's rectangle staged in LDS where it fits
    std::vector<std::vector<uint32_t>> uploads;  // the tables the last call that uploaded any built for its kernels: the sources of their copies (Staging::add_upload)
    int boxes_path = 0;             // option "boxes_path": 0 = kBoxesDefaultCombine decides; 1 = every lane its own atomics (yardstick); 2 = equal rows of a wave combined
    int hulls_path = 0;             // option "hulls_path": 0 = pwpp_hull_path_of decides; 1 = a lane per row, serial (yardstick); 2 = a wave per row
    bool ground_rows_valid = false;   // d_ground_rows holds the table of the last call (cleared by every estimate call and pwpp_trim_workspace)
    bool ground_query_queued = false;  // a PWPP_MEM_DEVICE query was enqueued on the main stream and nothing has waited for it yet
    DevBuf<uint32_t> d_bins{bufs, kPerBatch};  // 4 slabs of frames*(B+2): bin_count, bin_off, dst_a, dst_b
    DevBuf<uint32_t> d_parts{bufs, kPerBatch};  // TWO copies of 3 slabs of frames*(2B+2): part_count, part_off, part_cursor (pwpp_dev.h: a bin is stored in two
                               // parts); a call works on one copy while its K5 zeroes the other for the next call (PwppBatch.next_part_count)
    DevBuf<uint32_t> d_cls_start{bufs, kPerBatch};  // frames * 8
    DevBuf<uint32_t> d_cap_off{bufs, kPerHandle};  // 2B + 3 segment starts of the one-pass path (one segment per part)
    DevBuf<uint32_t> d_bin_max{bufs, kPerHandle};  // 2B + 2: largest count of every part so far (k_czm_scan)
    DevBuf<uint8_t> d_emit_long{bufs, kPerHandle};  // k_emit's table of long bins: B + 2 flags, then (4-byte aligned) the list of those bins as uint16
    std::vector<uint8_t> emit_long_flags;
    int emit_long_n = 0, emit_long_parts = 1;
    std::vector<uint32_t> observed, cap_table, cap_seen;  // host copies: d_bin_max as last read; capacities of the table on the device and the counts it was built from
    bool have_observation = false, table_stale = true;
    DevBuf<PwppFrameDesc> d_frames_probe{bufs, kPerBatch};
    PinnedBuf<uint32_t> h_bin_max{bufs, kPerHandle};
    DevBuf<uint16_t> d_cls_list{bufs, kPerBatch};  // frames * B
    DevBuf<PwppPatchRec> d_recs{bufs, kPerBatch};
    DevBuf<float> d_centers{bufs, kPerBatch}, d_normals{bufs, kPerBatch};
    DevBuf<PwppFrameResult> d_results{bufs, kPerBatch};  // two copies (see d_parts)
    int counters_copy = 0;           // which copy of d_parts / d_results the call in flight (or the last one) works on
    CleanCopy next_clean;            // the OTHER copy, if the last call's K5 zeroed it
    PinnedBuf<PwppFrameResult> h_results{bufs, kPerHandle};
    DevBuf<float> d_xyz{bufs, kPerBatch};  // gather scratch
    DevBuf<unsigned long long> d_dbg{bufs, kPerHandle};  // timing probes (PWPP_DEBUG_FLAGS & 4)

    // adaptive state: streams (long history slabs) and per-frame fresh outputs (short slabs)
    int num_streams = 0;
    int stream_hist_cap = 0, fresh_hist_cap = 0;
    int max_pushes_per_frame = 0;  // bins of the widest ring of interest: what one frame can add to a history
    DevBuf<PwppStateScalar> d_st_stream{bufs, kPerHandle}, d_st_fresh{bufs, kPerBatch};
    DevBuf<double> d_hist_stream{bufs, kPerHandle}, d_hist_fresh{bufs, kPerBatch};
    DevBuf<PwppPlaneState> d_pl_stream{bufs, kPerHandle}, d_pl_fresh{bufs, kPerBatch}, d_pl_snap{bufs, kPerBatch};  // the reference object's plane members after a frame (pwpp_dev.h)
    // one-pass batches of stateful streams: the state of the streams before the batch, so that a redo after an
    // overflow starts from it (the first attempt has already advanced sensor height, thresholds, histories)
    DevBuf<PwppStateScalar> d_st_snap{bufs, kPerBatch};
    DevBuf<double> d_hist_snap{bufs, kPerBatch};
};

namespace {

// The fixed-point contract of the plane-fit sums: every bin sums its points around an
// ORIGIN, its polar centre rounded to 1/8 m (a sector wider than a quarter turn keeps the sensor), and the
// shift s is the largest one <= 30 that keeps every point of every bin within 2^35 grid steps of its origin (contract v4, `wide`;
// v3 of rounds 3-5, option "exact_moments" = 0: <= 21 and 2^26).  Returns the z half-range ZR = 2^35 / 2^s (2^26 / 2^s) metres.
double fxp_geometry(const PwppDevParams &d, std::vector<float2> &origin, int &shift, bool wide) {
    double rmax = 0.0;
    origin.clear();
    for (int z = 0; z < 4; ++z)
        for (int r = 0; r < d.rings[z]; ++r)
            for (int k = 0; k < d.sectors[z]; ++k) {
                const double r0 = d.min_ranges[z] + r * d.ring_sizes[z];
                const double r1 = (z == 3 && r == d.rings[z] - 1) ? d.max_range : r0 + d.ring_sizes[z];
                const double t0 = k * d.sector_sizes[z], t1 = (k + 1) * d.sector_sizes[z];
                double cx = 0.0, cy = 0.0, far = r1;
                if (d.sectors[z] >= 4) {
                    const double rc = 0.5 * (r0 + r1), tc = 0.5 * (t0 + t1);
                    cx = std::rint(rc * std::cos(tc) * 8.0) / 8.0;
                    cy = std::rint(rc * std::sin(tc) * 8.0) / 8.0;
                    far = 0.0;
                    const double cr[2] = {r0, r1}, ct[2] = {t0, t1};
                    for (int a = 0; a < 2; ++a)
                        for (int b = 0; b < 2; ++b) {
                            const double dx = cr[a] * std::cos(ct[b]) - cx, dy = cr[a] * std::sin(ct[b]) - cy;
                            far = std::max(far, std::sqrt(dx * dx + dy * dy));
                        }
                }
                origin.push_back(make_float2((float)cx, (float)cy));
                rmax = std::max(rmax, far);
            }
    const double qmax = wide ? 34359738368.0 : 67108864.0;
    int s = wide ? 30 : 21;
    while (s > 0 && (rmax + 0.01) * (double)(1 << s) > qmax) --s;
    shift = s;
    return qmax / (double)(1 << s);
}

// Bounding box {xmin, xmax, ymin, ymax} of every bin: an annular sector reaches its extremes at its four corners or where
// it crosses an axis.  A little generous (1e-4 of the radius + 1 mm; the binning itself decides in double, and a point on
// the positive x axis belongs to the LAST sector, patchworkpp.cpp:570): the fit kernels only use it to prove that no point
// of a bin's high part can lie below a plane (stage_needs_hi, pwpp_fit.hip), so too large is safe and too small is not.
void bin_boxes(const PwppDevParams &d, std::vector<float4> &box) {
    box.clear();
    for (int z = 0; z < 4; ++z)
        for (int r = 0; r < d.rings[z]; ++r)
            for (int k = 0; k < d.sectors[z]; ++k) {
                const double r0 = d.min_ranges[z] + r * d.ring_sizes[z];
                const double r1 = (r == d.rings[z] - 1) ? (z == 3 ? d.max_range : d.min_ranges[z + 1]) : r0 + d.ring_sizes[z];
                const double t0 = k * d.sector_sizes[z], t1 = (k == d.sectors[z] - 1) ? 2 * M_PI : (k + 1) * d.sector_sizes[z];
                std::vector<double> th = {t0, t1};
                for (int q = 0; q <= 4; ++q)
                    if (q * (M_PI / 2) > t0 && q * (M_PI / 2) < t1) th.push_back(q * (M_PI / 2));
                double xmin = 1e300, xmax = -1e300, ymin = 1e300, ymax = -1e300;
                for (double t : th)
                    for (double rr : {std::min(r0, r1), std::max(r0, r1)}) {
                        xmin = std::min(xmin, rr * std::cos(t));
                        xmax = std::max(xmax, rr * std::cos(t));
                        ymin = std::min(ymin, rr * std::sin(t));
                        ymax = std::max(ymax, rr * std::sin(t));
                    }
                const double m = 1e-4 * std::max(r0, r1) + 1e-3;
                box.push_back(make_float4((float)(xmin - m), (float)(xmax + m), (float)(ymin - m), (float)(ymax + m)));
            }
}

int build_dev_params(const pwpp_params &p, PwppDevParams &d) {
    if (p.num_zones != 4)
        return fail(PWPP_E_UNSUPPORTED, "num_zones=%d: the reference hard-codes four zones (patchworkpp.h:122-134)", p.num_zones);
    if (p.num_iter < 1) return fail(PWPP_E_UNSUPPORTED, "num_iter=%d: must be >= 1", p.num_iter);
    if (p.num_lpr > PWPP_MAX_LPR) return fail(PWPP_E_UNSUPPORTED, "num_lpr=%d: at most %d supported", p.num_lpr, PWPP_MAX_LPR);
    if (p.num_rings_of_interest < 0 || p.num_rings_of_interest > PWPP_MAX_ROI)
        return fail(PWPP_E_ARG, "num_rings_of_interest=%d: the reference keeps update_*_[4] (patchworkpp.h:174-175)", p.num_rings_of_interest);
    if (!(p.max_range > p.min_range)) return fail(PWPP_E_ARG, "max_range must exceed min_range");
    if (!(p.max_range <= 8388607.0)) return fail(PWPP_E_UNSUPPORTED, "max_range=%g: at most 2^23 - 1 m supported", p.max_range);
    if (p.max_flatness_storage < 0 || p.max_elevation_storage < 0) return fail(PWPP_E_ARG, "negative history storage");
    std::memset(&d, 0, sizeof(d));
    int bins = 0, total_rings = 0, near = 0, max_near_sectors = 0;
    for (int k = 0; k < 4; ++k) {
        if (p.num_rings_each_zone[k] < 1 || p.num_sectors_each_zone[k] < 1)
            return fail(PWPP_E_ARG, "zone %d: rings and sectors must be >= 1", k);
        d.rings[k] = p.num_rings_each_zone[k];
        d.sectors[k] = p.num_sectors_each_zone[k];
        d.bin_base[k] = bins;
        for (int r = 0; r < d.rings[k]; ++r) {
            if (total_rings < p.num_rings_of_interest) {
                near += d.sectors[k];
                if (d.sectors[k] > max_near_sectors) max_near_sectors = d.sectors[k];
            }
            ++total_rings;
        }
        bins += d.rings[k] * d.sectors[k];
    }
    d.bin_base[4] = bins;
    if (bins > PWPP_MAX_BINS) return fail(PWPP_E_UNSUPPORTED, "%d CZM bins: at most %d supported", bins, PWPP_MAX_BINS);
    if (near > PWPP_MAX_NEAR_BINS) return fail(PWPP_E_UNSUPPORTED, "%d bins inside the rings of interest: at most %d", near, PWPP_MAX_NEAR_BINS);
    d.num_bins = bins;
    d.near_bins = near;
    // CZM geometry, the reference constructor's expressions in double (patchworkpp.h:122-134)
    const double mn = p.min_range, mx = p.max_range;
    const double z2 = (7 * mn + mx) / 8.0, z3 = (3 * mn + mx) / 4.0, z4 = (mn + mx) / 2.0;
    d.min_ranges[0] = mn;
    d.min_ranges[1] = z2;
    d.min_ranges[2] = z3;
    d.min_ranges[3] = z4;
    d.ring_sizes[0] = (z2 - mn) / p.num_rings_each_zone[0];
    d.ring_sizes[1] = (z3 - z2) / p.num_rings_each_zone[1];
    d.ring_sizes[2] = (z4 - z3) / p.num_rings_each_zone[2];
    d.ring_sizes[3] = (mx - z4) / p.num_rings_each_zone[3];
    for (int k = 0; k < 4; ++k) d.sector_sizes[k] = 2 * M_PI / p.num_sectors_each_zone[k];
    d.enable_RNR = p.enable_RNR != 0;
    d.enable_RVPF = p.enable_RVPF != 0;
    d.enable_TGR = p.enable_TGR != 0;
    d.num_iter = p.num_iter;
    d.num_lpr = p.num_lpr < 0 ? 0 : p.num_lpr;
    d.num_rings_of_interest = p.num_rings_of_interest;
    d.min_pts = (uint64_t)(size_t)p.num_min_pts;  // int -> size_t as in `size() < params_.num_min_pts` (patchworkpp.cpp:191)
    d.RNR_ver_angle_thr = p.RNR_ver_angle_thr;
    d.RNR_intensity_thr = p.RNR_intensity_thr;
    d.sensor_height = p.sensor_height;
    d.th_seeds = p.th_seeds;
    d.th_dist = p.th_dist;
    d.th_seeds_v = p.th_seeds_v;
    d.th_dist_v = p.th_dist_v;
    d.max_range = p.max_range;
    d.min_range = p.min_range;
    d.uprightness_thr = p.uprightness_thr;
    d.margin = p.adaptive_seed_selection_margin;
    d.fxp_shift = 0;  // (pwpp_create: fxp_geometry)
    d.f_min_range = (float)p.min_range;
    d.f_max_range = (float)p.max_range;
    d.f_margin_r = (float)(p.max_range * 1.5e-6 + 5e-5);  // metres; ~5x the float error budget of the radius
    d.f_margin_t = 8e-6f;                                  // radians; ~13x the error of the float angle
    for (int k = 0; k < 4; ++k) {
        d.f_zone[k] = (float)d.min_ranges[k];
        d.f_inv_ring[k] = (float)(1.0 / d.ring_sizes[k]);
        d.f_inv_sector[k] = (float)(1.0 / d.sector_sizes[k]);
    }
    d.max_elev_storage = p.max_elevation_storage;
    d.max_flat_storage = p.max_flatness_storage;
    for (int k = 0; k < 4; ++k) {
        d.elevation_thr0[k] = p.elevation_thr[k];
        d.flatness_thr0[k] = p.flatness_thr[k];
    }
    return max_near_sectors;  // >= 0
}

int use_device(pwpp_handle *h) {
    HIPCHK(hipSetDevice(h->device));
    return PWPP_OK;
}

void fill_default_state(const pwpp_handle *h, PwppStateScalar &s) {
    std::memset(&s, 0, sizeof(s));
    s.sensor_height = h->params.sensor_height;
    for (int k = 0; k < 4; ++k) {
        s.elevation_thr[k] = h->params.elevation_thr[k];
        s.flatness_thr[k] = h->params.flatness_thr[k];
    }
}

int finish_pending(pwpp_handle *h, bool lists_only = false);

// every stream a schedule may have put work on (error paths, pwpp_destroy): the main stream alone is not the join of a
// schedule that stopped half way
void sync_all_streams(pwpp_handle *h) {
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->aux_stream) (void)hipStreamSynchronize(h->aux_stream);
    for (hipStream_t st : h->extra_streams) (void)hipStreamSynchronize(st);
}

// the stream history slabs [stream][2][4][cap] re-laid out for a larger cap (contents kept)
int grow_stream_histories(pwpp_handle *h, int new_cap) {
    new_cap = (new_cap + 1) & ~1;  // (even: k_gle_tgr fetches two entries per load)
    const size_t rows = (size_t)h->num_streams * 8;
    std::vector<BufBase *> own;  // (a buffer of this function's, not yet the handle's)
    DevBuf<double> bigger{own, kPerHandle};
    int rc = bigger.ensure(rows * (size_t)new_cap);
    if (rc) return rc;
    HIPCHK(hipMemcpy2D(bigger.p, (size_t)new_cap * sizeof(double), h->d_hist_stream.p, (size_t)h->stream_hist_cap * sizeof(double),
                       (size_t)h->stream_hist_cap * sizeof(double), rows, hipMemcpyDeviceToDevice));
    bigger.swap(h->d_hist_stream);
    bigger.release();
    h->stream_hist_cap = new_cap;
    return PWPP_OK;
}

// Segment sizes of the one-pass path.  Round 6: a part's segment holds 1.0625 x the largest count that part has had in any frame
// this handle has seen (d_bin_max, kept by k_czm_scan; before the first batch a histogram of up to 256 sample frames fills it:
// probe_histogram) + 2 sqrt(that) + 16 slots, and every frame has an OVERFLOW ARENA behind its segments (pwpp_dev.h): a part that
// outgrows its segment is moved there by k_czm_scan, on the device, at the cost of a copy of that part -- ~1.7 slots per point of a
// KITTI frame, 27 B per point.  (Rounds 2-5: 1.5 x + 256 slots and no arena -- 2.7 slots per point, every overflow a frame binned
// twice by the host; round 1: 20 slots per point.)  one_pass_scale scales the 1.0625 (tests use a tiny one to force overflows).
// A frame whose arena runs out raises the overflow flag and is binned again on the exact two-pass path, whose counts enter
// d_bin_max, and the table is rebuilt.
int build_capacity_table(pwpp_handle *h, int max_n) {
    const PwppDevParams &P = h->dp;
    const int NB = PWPP_NUM_PARTS(P.num_bins);  // one segment per part
    // A FEW frames per call (a single sensor's stream, the reference's own use): memory is no concern there (2 048 slots more per part
    // are 40 MB per frame), but every overflow is a frame binned twice (these calls get no arena), and a handle that has seen a
    // handful of frames knows little about its bins -- 3.75 x the largest count + 2048.
    const bool few = h->frames <= 16 && h->one_pass_scale >= 1.0;
    h->cap_few = few;
    const double scale = (few ? 3.75 : 1.0625) * h->one_pass_scale / 4.0;
    std::vector<uint32_t> off((size_t)NB + 1);
    h->cap_table.assign((size_t)NB, 0u);
    h->cap_seen = h->observed;
    uint64_t run = 0;
    for (int b = 0; b < NB; ++b) {
        off[(size_t)b] = (uint32_t)run;
        const double seen = (double)h->observed[(size_t)b];
        double cap = scale * seen + (h->one_pass_scale >= 1.0 ? (few ? 2048.0 : 2.0 * std::sqrt(seen) + 16.0) : 16.0);
        if (cap > (double)max_n + 16.0) cap = (double)max_n + 16.0;
        uint64_t c = ((uint64_t)cap + (PWPP_SLOT_ALIGN - 1)) & ~(uint64_t)(PWPP_SLOT_ALIGN - 1);
        if (b < 2 * P.num_bins && (b & 1) && b / 2 >= P.split_end) c = 0;  // the high part of a bin that is not split: never used
        h->cap_table[(size_t)b] = (uint32_t)c;
        run += c;
        if (run >= ((uint64_t)1 << 31)) return fail(PWPP_E_NOMEM, "one-pass capacity table overflows 31-bit offsets");
    }
    off[(size_t)NB] = (uint32_t)run;
    // the arena: room for the largest part to move as a whole, plus a sixteenth of the largest frame -- 4 096 slots at least; a
    // quarter of it (2 048 at least) may fill with spilled records
    uint64_t arena = 0;
    if (!few && !(h->debug_flags & 2048)) {  // (debug 2048: no arena -- rounds 2-5's behaviour on today's segments, for tests and A/B runs)
        uint32_t biggest = 0;
        for (int b = 0; b < NB; ++b) biggest = h->observed[(size_t)b] > biggest ? h->observed[(size_t)b] : biggest;
        arena = (uint64_t)biggest + biggest / 4 + (uint64_t)max_n / 16 + 4096;
        if (h->one_pass_scale < 1.0) arena = (uint64_t)((double)arena * h->one_pass_scale);  // (tests: a small arena overflows too)
        arena = (arena + (PWPP_SLOT_ALIGN - 1)) & ~(uint64_t)(PWPP_SLOT_ALIGN - 1);
        if (run + arena >= ((uint64_t)1 << 31)) arena = 0;
    }
    int rc = h->d_cap_off.ensure((size_t)NB + 1);
    if (rc) return rc;
    HIPCHK(hipMemcpy(h->d_cap_off.p, off.data(), off.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    h->arena_base = (uint32_t)run;
    h->arena_slots = (uint32_t)arena;
    h->arena_spill = (uint32_t)(arena / 4 > 2048 ? arena / 4 : (arena < 2048 ? arena : 2048));
    h->slots_per_frame = (int64_t)(run + arena);
    h->cap_max_n = max_n;
    h->table_stale = false;
    return PWPP_OK;
}

void fill_batch(pwpp_handle *h, PwppBatch &bt);
// Words of ONE copy of the part counters (part_count, part_off, part_cursor: three slabs of frames x parts words).  A multiple of
// four words with four to spare: k_clear zeroes whole 16-byte words from the copy's first word, so the SECOND copy must start
// on a 16-byte boundary too (3 x frames x parts + 4 is 8 mod 16 bytes for a single frame of the default CZM).
inline size_t counters_copy_words(size_t slab_words) { return (3 * slab_words + 4 + 3) & ~(size_t)3; }

constexpr unsigned bit(Output o) { return 1u << o; }
// what the next call writes: the settings, and the labels that PWPP_ORDER_CLOUD implies
unsigned outputs_on(const pwpp_handle *h) { return h->outputs | (h->output_order == PWPP_ORDER_CLOUD ? bit(kLabels) : 0u); }
bool labels_on(const pwpp_handle *h) { return outputs_on(h) & bit(kLabels); }
int64_t label_tile_stride(int max_n) { return ((int64_t)max_n + 15 + PWPP_LABEL_TILE - 1) / PWPP_LABEL_TILE; }

int read_observed(pwpp_handle *h) {
    const size_t NB = (size_t)PWPP_NUM_PARTS(h->dp.num_bins);
    h->observed.resize(NB);
    HIPCHK(hipMemcpy(h->observed.data(), h->d_bin_max.p, NB * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return PWPP_OK;
}

// Histogram of up to 256 frames spread over the batch described by h->descs (inputs already on their way to the device):
// K0 + K1 + K2 on a private descriptor array, which leaves the bins' largest counts in d_bin_max.
int probe_histogram(pwpp_handle *h) {
    // (round 5: up to 256 sample frames -- with 32, 353 of the first 512 frames of a varied drive outgrew some segment (bench.py,
    // `distinct` leg); the probe is a histogram pass, ~1 us per frame)
    const int S = h->frames < 256 ? h->frames : 256;
    std::vector<PwppFrameDesc> sample((size_t)S);
    int max_n = 0;
    for (int i = 0; i < S; ++i) {
        // (scattered over the batch, not evenly spaced: replayed or periodic inputs would alias with a fixed stride)
        const size_t pick = S == h->frames ? (size_t)i : (size_t)(((uint64_t)(i + 1) * 2654435761ull) % (uint64_t)h->frames);
        sample[(size_t)i] = h->descs[pick];
        if (h->mode != PWPP_MODE_FRESH) sample[(size_t)i].state_in = sample[(size_t)i].state_out;  // (RNR reads the stream's sensor height)
        sample[(size_t)i].state_out = i;  // never written: the probe stops after K2
        if (sample[(size_t)i].n > max_n) max_n = sample[(size_t)i].n;
    }
    int rc = h->d_frames_probe.ensure((size_t)S);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(h->d_frames_probe.p, sample.data(), (size_t)S * sizeof(PwppFrameDesc), hipMemcpyHostToDevice, h->stream));
    PwppBatch bt;
    fill_batch(h, bt);
    bt.frames = h->d_frames_probe.p;
    bt.num_frames = S;
    bt.max_n = max_n;
    bt.cap_off = nullptr;
    h->next_clean.valid = false;  // (the probe's own K0-K2 run on sample frames with their own frame count)
    bt.next_part_count = nullptr;
    const int lrc = pwpp_launch_histogram(&bt, h->stream);
    if (lrc != 0) return fail(PWPP_E_HIP, "histogram probe failed: %s", hipGetErrorString((hipError_t)lrc));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->have_observation = true;
    return read_observed(h);
}

// k_emit's table of "long" bins (pwpp_dev.h: emit_long) from the parts' largest counts so far; uploaded when it changes.
// Called with no launch in flight (estimate_batch, after finish_pending).
int refresh_emit_long(pwpp_handle *h) {
    const int B = h->dp.num_bins, NB = B + 2;
    std::vector<uint8_t> flag((size_t)NB, 0);
    std::vector<uint16_t> list;
    uint32_t biggest = 0;
    for (int b = 0; b < NB && h->observed.size() == (size_t)PWPP_NUM_PARTS(B) && !(h->debug_flags & 1024); ++b) {  // (debug 1024: no long-list table)
        const uint32_t c = b < B ? h->observed[2 * (size_t)b] + h->observed[2 * (size_t)b + 1] : h->observed[(size_t)B + b];  // (pseudo-bin s = part B + s)
        if (c > PWPP_EMIT_LONG_MIN) {
            flag[(size_t)b] = 1;
            list.push_back((uint16_t)b);
            biggest = c > biggest ? c : biggest;
        }
    }
    int parts = (int)((biggest > 512u * PWPP_EMIT_LONG_BLOCKS ? biggest - 512u * PWPP_EMIT_LONG_BLOCKS : 0u) / 4096u) + 1;
    parts = parts > 32 ? 32 : parts;
    if (flag == h->emit_long_flags && parts == h->emit_long_parts) return PWPP_OK;
    const size_t list_at = (size_t)((NB + 3) & ~3);
    std::vector<uint8_t> blob(list_at + 2 * (size_t)NB, 0);
    std::memcpy(blob.data(), flag.data(), flag.size());
    if (!list.empty()) std::memcpy(blob.data() + list_at, list.data(), list.size() * sizeof(uint16_t));
    int rc = h->d_emit_long.ensure(blob.size());
    if (rc) return rc;
    HIPCHK(hipMemcpy(h->d_emit_long.p, blob.data(), blob.size(), hipMemcpyHostToDevice));
    h->emit_long_flags = flag;
    h->emit_long_n = (int)list.size();
    h->emit_long_parts = parts;
    return PWPP_OK;
}

// everything a launch needs except the frame range, the capacity table and the events
void fill_batch(pwpp_handle *h, PwppBatch &bt) {
    const int B = h->dp.num_bins, NB = B + 2;
    std::memset(&bt, 0, sizeof(bt));
    bt.P = h->dp;
    bt.frames = h->d_frames.p;
    bt.num_frames = h->frames;
    bt.max_n = h->max_n;
    bt.debug = h->debug_flags;
    bt.fit_plan = h->fit_plan.empty() ? nullptr : h->fit_plan.c_str();
    bt.plan_frames = 0;
    if (h->mode == PWPP_MODE_FRESH) {
        bt.P.hist_cap = h->fresh_hist_cap;
        bt.st_scalar = h->d_st_fresh.p;
        bt.st_hist = h->d_hist_fresh.p;
        bt.st_plane = h->d_pl_fresh.p;
    } else {
        bt.P.hist_cap = h->stream_hist_cap;
        bt.st_scalar = h->d_st_stream.p;
        bt.st_hist = h->d_hist_stream.p;
        bt.st_plane = h->d_pl_stream.p;
    }
    bt.codes = h->d_codes.p;
    const size_t slab = (size_t)h->frames * NB, pslab = (size_t)h->frames * PWPP_NUM_PARTS(B);
    bt.bin_count = h->d_bins.p;
    bt.bin_off = h->d_bins.p + slab;
    bt.dst_a = h->d_bins.p + 2 * slab;
    bt.dst_b = h->d_bins.p + 3 * slab;
    const size_t pcopy = counters_copy_words(pslab);
    uint32_t *parts = h->d_parts.p + (size_t)h->counters_copy * pcopy;
    bt.part_count = parts;
    bt.part_off = parts + pslab;
    bt.part_cursor = parts + 2 * pslab;
    bt.next_part_count = h->d_parts.p + (size_t)(h->counters_copy ^ 1) * pcopy;
    bt.next_results = h->d_results.p + (size_t)(h->counters_copy ^ 1) * (size_t)h->frames;
    bt.next_slab_stride = (int64_t)pslab;
    bt.next_slabs = 3;  // (launch_prepared narrows it to 1 for a one-pass batch)
    bt.cls_start = h->d_cls_start.p;
    bt.cls_list = h->d_cls_list.p;
    bt.sorted_z = h->d_sorted_z.p;
    bt.sorted_xy = h->d_sorted_xy.p;
    bt.sorted_idx = h->d_sorted_idx.p;
    bt.bin_origin = h->d_bin_origin.p;
    bt.bin_bbox = h->d_bin_bbox.p;
    bt.member = h->d_member.p;
    bt.order_work = h->output_order == PWPP_ORDER_REFERENCE ? h->d_ord_work.p : nullptr;
    bt.recs = h->d_recs.p;
    bt.out_idx = h->d_out.p;
    bt.centers = h->d_centers.p;
    bt.normals = h->d_normals.p;
    bt.results = h->d_results.p + (size_t)h->counters_copy * (size_t)h->frames;
    bt.results_host = h->h_results.p;  // hipHostMalloc'ed: the same address on the device
    bt.dbg = h->d_dbg.p;
    const unsigned outputs = outputs_on(h);
    if (outputs & (bit(kLabels) | bit(kPointPlanes))) {
        bt.point_first = 0;
        bt.point_count = h->h_base.p[h->frames];
    }
    if (outputs & bit(kPointPlanes)) {
        bt.pt_patch = h->d_pt_patch.p;
        bt.pt_dist = h->d_pt_dist.p;
        bt.pt_rows = h->d_pt_rows.p;
    }
    if (outputs & bit(kPointRecords)) {
        bt.records = h->d_records.p;
        bt.record_bytes = h->record_bytes;
        bt.records_path = h->records_path;
    }
    if (outputs & bit(kLabels)) {
        bt.labels = h->d_labels.p;
        if (h->output_order == PWPP_ORDER_CLOUD) {
            bt.label_tiles = h->d_label_tiles.p;
            bt.label_tile_stride = (int32_t)label_tile_stride(h->max_n);
        }
    }

    bt.bin_max = h->d_bin_max.p;
    bt.arena_base = 0xffffffffu;  // (launch_prepared sets the arena of a one-pass batch)
    bt.arena_slots = bt.arena_spill = 0u;
    bt.arena_tag = nullptr;
    {   // k_emit: one wave per bin copies a list of a few thousand entries well; the bins of a dense cloud get more
        uint32_t biggest = 0;  // (observed: per part; a bin's two parts are neighbours, the pseudo-bins the last two entries)
        for (size_t b = 0; b + 1 < h->observed.size(); b += 2) {
            const uint32_t both = b < 2 * (size_t)B ? h->observed[b] + h->observed[b + 1] : (h->observed[b] > h->observed[b + 1] ? h->observed[b] : h->observed[b + 1]);
            biggest = both > biggest ? both : biggest;
        }
        int parts = (int)(biggest / 8192u) + 1;
        // a few frames: the kernel is as long as the copy of its longest list by ONE wave (a 4 900-point patch: ten rounds of
        // 512 entries, ~1 us each) -- eight waves per bin cut that chain (single frame: k_emit 13.2 -> see DESIGN.md), where a
        // big batch would only pay for the empty waves (0.24 -> 0.30 ms with two per bin)
        if (h->frames <= 8) parts = 8;
        else if (h->frames <= 64 && parts < 4) parts = 4;
        bt.emit_parts = parts > 8 ? 8 : parts;
        if (h->frames > 64) {
            // Big batches (round 5): ONE wave per bin, and extra waves only for the bins that have held more than PWPP_EMIT_LONG_MIN
            // entries in some frame of this handle (refresh_emit_long: a table on the device, rebuilt when the maxima change).
            // A long list in a bin that is not in the table yet is copied whole by its one wave: slower, never wrong.
            bt.emit_parts = 1;
            if (h->emit_long_n > 0) {
                bt.emit_long = h->d_emit_long.p;
                bt.emit_long_list = reinterpret_cast<const uint16_t *>(h->d_emit_long.p + (size_t)((B + 2 + 3) & ~3));
                bt.emit_long_n = h->emit_long_n;
                bt.emit_long_parts = h->emit_long_parts;
            }
        }
    }
}

// a view of the batch's workspaces that covers the frames [f0, f0 + nf): every per-frame array is indexed by the frame
PwppBatch frame_range(const pwpp_handle *h, const PwppBatch &bt, int f0, int nf) {
    const int B = h->dp.num_bins, NB = B + 2, NP = PWPP_NUM_PARTS(B);
    PwppBatch v = bt;
    v.frames += f0;
    v.num_frames = nf;
    v.no_clear = 1;
    v.bin_count += (size_t)f0 * NB;
    v.bin_off += (size_t)f0 * NB;
    v.part_count += (size_t)f0 * NP;
    v.part_off += (size_t)f0 * NP;
    v.part_cursor += (size_t)f0 * NP;
    v.dst_a += (size_t)f0 * NB;
    v.dst_b += (size_t)f0 * NB;
    v.cls_start += (size_t)f0 * PWPP_CLS_STRIDE;
    v.cls_list += (size_t)f0 * B;
    v.recs += (size_t)f0 * B;
    v.centers += (size_t)f0 * B * 3;
    v.normals += (size_t)f0 * B * 3;
    v.results += f0;
    v.results_host += f0;
    if (v.order_work) v.order_work += (size_t)f0 * (size_t)(1 + 2 * NB);
    if (v.arena_tag) v.arena_tag += (size_t)f0 * v.arena_spill;
    if (v.labels || v.pt_patch) {
        v.point_first = h->h_base.p[f0];
        v.point_count = h->h_base.p[f0 + nf] - h->h_base.p[f0];
    }
    if (v.pt_rows) v.pt_rows += (size_t)f0 * B;
    if (v.label_tiles) v.label_tiles += (size_t)f0 * (size_t)v.label_tile_stride;
    v.next_part_count += (size_t)f0 * NP;  // (the other copy: same frame, same slab stride)
    v.next_results += f0;
    return v;
}

void CleanCopy::capture(const pwpp_handle *h, int frames_, int slabs_) {
    valid = true;
    frames = frames_;
    slabs = slabs_;
    parts = h->d_parts.p;
    results = h->d_results.p;
    parts_cap = h->d_parts.cap;
    results_cap = h->d_results.cap;
}
bool CleanCopy::matches(const pwpp_handle *h, int frames_, int slabs_) const {
    return valid && frames == frames_ && slabs >= slabs_ && parts == h->d_parts.p && results == h->d_results.p &&
           parts_cap == h->d_parts.cap && results_cap == h->d_results.cap;
}

// the overflow arena of the current capacity table (one-pass layout), for a view that starts at frame f0
void set_arena(const pwpp_handle *h, PwppBatch &v, int f0) {
    v.arena_base = h->arena_base;
    v.arena_slots = h->arena_slots;
    v.arena_spill = h->arena_spill;
    v.arena_tag = h->arena_slots ? h->d_arena_tag.p + (size_t)f0 * h->arena_spill : nullptr;
}

// nothing of a half-launched schedule may still be running when the caller sees the error
int launch_failed(pwpp_handle *h, int lrc) {
    sync_all_streams(h);
    return fail(PWPP_E_HIP, "kernel launch failed: %s", hipGetErrorString((hipError_t)lrc));
}

// the stages of one pipeline on the main stream.  whole_call: a call's own launch, with the profiling events and the second
// stream of the latency plan; a redo or a fix-up runs without them.
int launch_pipeline(pwpp_handle *h, const PwppBatch &v, int stages, bool whole_call = false) {
    const bool ordered = h->output_order == PWPP_ORDER_REFERENCE;
    const int lrc = pwpp_launch_pipeline(&v, h->stream, whole_call && h->profiling ? h->ev_k : nullptr, whole_call ? h->aux_stream : nullptr,
                                         whole_call ? h->aux_fork : nullptr, whole_call ? h->aux_join : nullptr,
                                         ordered ? h->d_ord_a.p : nullptr, ordered ? h->d_ord_b.p : nullptr, stages);
    return lrc != 0 ? launch_failed(h, lrc) : PWPP_OK;
}

// Launches the pipeline over the batch described by h->descs (buffers sized, inputs on the device).
// one_pass: fixed bin segments (k_czm_bin_scatter); otherwise the exact two-pass binning.
int launch_prepared(pwpp_handle *h, bool one_pass) {
    const int NP = PWPP_NUM_PARTS(h->dp.num_bins);
    const int frames = h->frames;
    if (h->k5_tail_unjoined) {  // the threshold update of the streams' last frames (K5's second part) comes before anything of this call
        HIPCHK(hipStreamWaitEvent(h->stream, h->aux_join, 0));
        h->k5_tail_unjoined = false;
    }
    // where a frame's bins live in the bin-ordered buffers
    int64_t base = 0;
    for (int f = 0; f < frames; ++f) {
        PwppFrameDesc &d = h->descs[(size_t)f];
        d.sbase = one_pass ? (int64_t)f * h->slots_per_frame : base;
        d.mbase = d.sbase / 8 + (int64_t)2 * PWPP_MEMBER_PAD * NP * f;  // (sbase is a multiple of PWPP_SLOT_ALIGN in both layouts; a pad per part, and one more for a part moved into the arena)
        // compact layout: every part starts at a multiple of PWPP_SLOT_ALIGN slots (k_czm_scan)
        base += ((int64_t)d.n + (PWPP_SLOT_ALIGN - 1) * (int64_t)NP + (PWPP_SLOT_ALIGN - 1)) & ~(int64_t)(PWPP_SLOT_ALIGN - 1);
    }
    // the descriptors on the device are reused when nothing changed (a caller cycling through the same
    // device buffers, a replayed batch): one host-to-device copy less in front of the first kernel
    const size_t desc_bytes = (size_t)frames * sizeof(PwppFrameDesc);
    if (h->descs_on_device.size() != (size_t)frames || h->descs_dev_ptr != h->d_frames.p ||
        std::memcmp(h->descs_on_device.data(), h->descs.data(), desc_bytes) != 0) {
        std::memcpy(h->h_frames.p, h->descs.data(), desc_bytes);
        HIPCHK(hipMemcpyAsync(h->d_frames.p, h->h_frames.p, desc_bytes, hipMemcpyHostToDevice, h->stream));
        h->descs_on_device = h->descs;
        h->descs_dev_ptr = h->d_frames.p;
    }

    // this call works on the other copy of the counters; if the last call's K5 zeroed exactly what this one needs, no
    // clearing kernel runs in front of the binning
    h->counters_copy ^= 1;
    const int slabs = one_pass ? 1 : 3;
    const bool pre_cleared = h->next_clean.matches(h, frames, slabs);
    h->next_clean.valid = false;  // (set again below, once this call's K5 is on its way for every frame)
    PwppBatch bt;
    fill_batch(h, bt);
    bt.next_slabs = slabs;
    bt.no_clear = pre_cleared ? 1 : 0;

    // A few stateful streams (the latency plan): the index lists wait for the first part of K5 only; the statistics over the streams'
    // histories -- what only their NEXT frames need -- run on aux_stream under K6 and the host's turn-around.
    const bool split_k5 = h->split_k5 != 0 && h->mode == PWPP_MODE_STREAMS && frames <= 64 && !h->profiling && bt.debug == 0 &&
                          h->output_order != PWPP_ORDER_REFERENCE && h->dp.min_pts != 0;
    bt.k5_split = split_k5 ? h->split_k5 : 0;
    bt.cap_off = one_pass ? h->d_cap_off.p : nullptr;
    if (one_pass) set_arena(h, bt, 0);
    if (one_pass && h->mode == PWPP_MODE_STREAMS) {  // what a redo after a segment overflow starts from: copied by the binning kernel
        bt.snap_scalar = h->d_st_snap.p;
        bt.snap_hist = h->d_hist_snap.p;
        bt.snap_plane = h->d_pl_snap.p;
    }
    if (pre_cleared && (bt.debug & 64)) {
        // the pre-cleared path rests on every K5 variant zeroing the OTHER copy of the counters for every frame.
        // Debug option: read this call's copy back before the binning touches it; anything but zeros is a broken invariant.
        HIPCHK(hipStreamSynchronize(h->stream));
        const size_t words = (size_t)slabs * (size_t)frames * (size_t)PWPP_NUM_PARTS(h->dp.num_bins);
        std::vector<uint32_t> hp(words);
        std::vector<PwppFrameResult> hr((size_t)frames);
        HIPCHK(hipMemcpy(hp.data(), bt.part_count, words * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(hr.data(), bt.results, hr.size() * sizeof(PwppFrameResult), hipMemcpyDeviceToHost));
        size_t bad = 0;
        for (uint32_t v : hp) bad += v != 0u;
        const unsigned char *rb = reinterpret_cast<const unsigned char *>(hr.data());
        for (size_t i = 0; i < hr.size() * sizeof(PwppFrameResult); ++i) bad += rb[i] != 0;
        if (bad) return fail(PWPP_E_STATE, "pre-cleared counters are not zero (%zu words / bytes): a K5 variant skipped clear_next_counters", bad);
    }
    HIPCHK(hipEventRecord(h->ev_begin, h->stream));
    // (the histogram, the scatter cursors and the per-frame result counters are zeroed by the pipeline's
    // first kernel, k_clear)
    if (bt.debug & 4) {
        HIPCHK(hipMemsetAsync(bt.dbg, 0, 64 * sizeof(unsigned long long), h->stream));
        HIPCHK(hipMemsetAsync(bt.dbg + 60, 0xFF, sizeof(unsigned long long), h->stream));  // slot 60 is a minimum
    }
    // Overlap mode: the pipeline alternates memory-bound stages (binning, emit) and VALU-bound ones (the
    // fits).  Two halves of the batch, each with its own launches on its own stream, put one kind under the
    // other (tools/two_handles.py: +7.5 % on 1024 KITTI frames).  Every per-frame array is indexed by the
    // frame, so the halves are two views of the same workspaces with shifted base pointers.
    const bool overlapped = h->overlap && !h->profiling && h->output_order != PWPP_ORDER_REFERENCE && frames >= 128 && bt.debug == 0;
    if (overlapped) {
        auto range = [&](int f0, int nf) { return frame_range(h, bt, f0, nf); };
        // R frame ranges of whole groups of eight frames (K1' deals frames to the 8 XCDs).  Every range is launched
        // with the fit plan of the WHOLE batch (the machine is shared, not split).
        int R = h->overlap_ranges < 2 ? 2 : h->overlap_ranges;
        while (R > 2 && frames / R < 64) --R;
        // big bins per wave: four on scans of KITTI density (+2 % over two in interleaved end-to-end runs), two where the
        // bins are several times larger (dense 128-beam frames, 36-sector CZM: 110.9 k against 106.8 k frames/s)
        bt.plan_frames = frames;  // (pwpp_launch_fit picks the plan; round 4: also below 640 frames -- the ranges used to pick one for their own size)
        std::vector<int> first((size_t)R + 1, 0);
        for (int r = 1; r <= R; ++r) {
            int f1 = r == R ? frames : (int)(((int64_t)frames * r / R + 7) / 8 * 8);
            first[(size_t)r] = f1 > frames ? frames : f1;
        }
        int lrc = pre_cleared ? 0 : pwpp_launch_clear(&bt, h->stream);
        // A software pipeline over the two streams: the MEMORY stream bins range r + 2 and then writes the lists of
        // range r, the FIT stream runs the plane fits (and K5) of range r + 1 meanwhile -- the streams never run the
        // same kind of stage at the same time (two whole-range pipelines side by side start in lock step: both
        // binning, then both fitting).  Events: range binned -> its fits may start; range fitted -> its lists.
        while (h->ev_ranges.size() < 2 * (size_t)R) {
            hipEvent_t e = nullptr;
            HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            h->ev_ranges.push_back(e);
        }
        auto stage = [&](int r, int stages, hipStream_t st) {
            if (lrc != 0 || first[(size_t)r + 1] <= first[(size_t)r]) return;
            const PwppBatch v = range(first[(size_t)r], first[(size_t)r + 1] - first[(size_t)r]);
            lrc = pwpp_launch_pipeline(&v, st, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, stages);
        };
        // (the fit stages go round a few streams: a fit kernel ends with the tail of its longest waves, and the next
        // range's kernels fill the machine meanwhile)
        while ((int)h->extra_streams.size() + 1 < h->num_fit_streams) {
            hipStream_t st = nullptr;
            HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
            h->extra_streams.push_back(st);
        }
        const hipStream_t mem = h->stream;
        // (every record / wait is checked: a failed one would leave the fit streams unordered against binning and
        // k_emit, and the batch would "succeed" with racy results -- ADVICE r02)
        auto ordered_ok = [&](hipError_t e) {
            if (e != hipSuccess && lrc == 0) lrc = (int)e;
        };
        auto bin = [&](int r) {
            const int k = r % h->num_fit_streams;
            hipStream_t fit = k == 0 ? h->aux_stream : h->extra_streams[(size_t)k - 1];
            stage(r, 1, mem);
            if (lrc == 0) ordered_ok(hipEventRecord(h->ev_ranges[2 * (size_t)r], mem));
            if (lrc == 0) ordered_ok(hipStreamWaitEvent(fit, h->ev_ranges[2 * (size_t)r], 0));
            stage(r, 2, fit);
            if (lrc == 0) ordered_ok(hipEventRecord(h->ev_ranges[2 * (size_t)r + 1], fit));
        };
        auto lists = [&](int r) {
            if (lrc == 0) ordered_ok(hipStreamWaitEvent(mem, h->ev_ranges[2 * (size_t)r + 1], 0));
            stage(r, 4, mem);
        };
        bin(0);
        if (R > 1) bin(1);
        for (int r = 0; r < R; ++r) {
            lists(r);
            if (r + 2 < R) bin(r + 2);
        }
        // (the memory stream ends with the lists of the last range, which wait for its fits: h->stream is the join)
        if (lrc != 0) return launch_failed(h, lrc);
    } else if (const int rc = launch_pipeline(h, bt, 7, true)) {
        return rc;
    }
    HIPCHK(hipEventRecord(h->ev_end, h->stream));
    if (bt.k5_split && !overlapped) {
        if (bt.k5_split == 2) {  // the second part behind the lists
            HIPCHK(hipEventRecord(h->aux_fork, h->stream));
            const int trc = pwpp_launch_k5_tail(&bt, h->aux_stream, h->aux_fork, h->aux_join);
            if (trc != 0) return launch_failed(h, trc);
        }
        h->k5_tail_unjoined = h->k5_tail_unsynced = true;
    }
    h->next_clean.capture(h, frames, slabs);  // every frame's K5 is enqueued: the other copy will be zero for a call of this shape
    if (one_pass)  // the bins' largest counts, for the segment sizes of the next batches (finish_pending)
        HIPCHK(hipMemcpyAsync(h->h_bin_max.p, h->d_bin_max.p, (size_t)NP * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    h->profile_pending = h->profiling;
    h->one_pass = one_pass;
    g_slot0_one_pass = one_pass;
    return PWPP_OK;
}

// What K5's second launch (split_k5) leaves behind the index lists: the streams' state, and how full their histories are.
int settle_k5_tail(pwpp_handle *h) {
    if (h->k5_tail_unsynced) {  // (the streams' state and results[].hist_state are complete once K5's second part has run)
        HIPCHK(hipStreamSynchronize(h->aux_stream));
        h->k5_tail_unsynced = false;
    }
    if (h->hist_check_due) {
        h->hist_check_due = false;
        // The reference's history vectors are unbounded (update_flatness_thr stops trimming the higher rings while a
        // lower one holds <= 1 entries, patchworkpp.cpp:363-364).  The slabs grow before a call could fill them.
        int fill = 0;
        bool dropped = false;
        for (int f = 0; f < h->frames; ++f) {
            const int hs = h->h_results.p[f].hist_state;
            fill = (hs >> 1) > fill ? (hs >> 1) : fill;
            dropped = dropped || (hs & 1);
        }
        if (dropped) return fail(PWPP_E_STATE, "an A-GLE history outgrew its slab (%d entries): the adaptive thresholds of this stream are no longer the reference's", h->stream_hist_cap);
        if (fill + h->max_pushes_per_frame + 8 > h->stream_hist_cap) {
            const int rc = grow_stream_histories(h, 2 * h->stream_hist_cap);
            if (rc) return rc;
        }
    }
    return PWPP_OK;
}

// lists_only (pwpp_synchronize, the getters of a call's results, pwpp_get_time_us): the caller wants what the main stream delivers -- counts,
// index lists, patch rows.  K5's second launch may then stay on its stream (the next estimate call and everything that touches a stream's
// state settle it first), unless a frame of the call needs the host: a redo or a fix-up restores / continues the streams' state.
int finish_pending(pwpp_handle *h, bool lists_only) {
    if (!h->pending) return lists_only ? PWPP_OK : settle_k5_tail(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    bool defer_tail = lists_only && h->k5_tail_unsynced;
    for (int f = 0; f < h->frames && defer_tail; ++f)
        if (h->h_results.p[f].overflow & 3) defer_tail = false;
    if (h->k5_tail_unsynced && !defer_tail) {
        HIPCHK(hipStreamSynchronize(h->aux_stream));
        h->k5_tail_unsynced = false;
    }
    h->pending = false;
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, h->ev_begin, h->ev_end));
    h->time_us = (double)ms * 1000.0;
    if (h->profile_pending) {
        for (int k = 0; k < PWPP_NUM_KERNELS; ++k) {
            float kms = 0.0f;
            HIPCHK(hipEventElapsedTime(&kms, h->ev_k[k], h->ev_k[k + 1]));
            h->prof_ms[k] += kms;
            h->prof_launches[k] += 1;
        }
        h->profile_pending = false;
    }
    const bool was_one_pass = h->one_pass;
    bool redone_in_place = false;
    if (h->one_pass) {  // did every bin of every frame fit its segment?  the frames that did not are redone on the exact two-pass path
        std::vector<int> redo;
        for (int f = 0; f < h->frames; ++f)
            if (h->h_results.p[f].overflow & 1) redo.push_back(f);
        h->one_pass = false;
        h->frame_two_pass.assign((size_t)h->frames, 0);
        if (!redo.empty()) {
            {   // the exact path needs the per-point codes (not held for one-pass batches)
                const int rc = h->d_codes.ensure((size_t)(h->total_points > 0 ? h->total_points : 1));
                if (rc) return rc;
            }
            ++h->one_pass_redone;
            h->one_pass_holdoff = 0;  // (the redo's exact counts enter d_bin_max and the table is rebuilt: no need to stay away)
            h->table_stale = true;
            // A frame is redone IN PLACE: its compact two-pass layout (points + the parts' alignment pads) starts at the frame's own
            // first slot of the one-pass layout, whose segments are ~2.7 slots per point -- the other frames of the batch are not
            // touched (frames are independent: fresh state, or one stream each).  Only a frame that would not fit its own
            // slots (a table built from much smaller frames) sends the whole batch through the compact layout.
            const int NP = PWPP_NUM_PARTS(h->dp.num_bins);
            bool in_place = !h->redo_whole_batch;
            {   //  every run of neighbouring frames is a pipeline of its own -- four memsets and ten small launches, one after
                // the other on one stream.  A cold or out-of-distribution batch with overflows all over it (353 of 512 frames once) is
                // cheaper as ONE whole-batch redo on the two-pass path (~2.5 ms per 1024 frames) than as hundreds of those.
                size_t runs = 0;
                for (size_t i = 0; i < redo.size(); ++i) runs += i == 0 || redo[i] != redo[i - 1] + 1;
                if (runs > 16 && (redo.size() > (size_t)h->frames / 8 || runs > 64)) in_place = false;
            }
            for (int f : redo) {
                const int64_t need = (int64_t)h->descs[(size_t)f].n + (int64_t)(PWPP_SLOT_ALIGN - 1) * NP + PWPP_SLOT_ALIGN;
                if (need > h->slots_per_frame) in_place = false;
            }
            if (h->mode == PWPP_MODE_STREAMS) {  // back to the state before the first attempt -- of the streams that are redone
                const size_t slab = (size_t)8 * (size_t)h->stream_hist_cap;
                if (!in_place) {
                    HIPCHK(hipMemcpyAsync(h->d_st_stream.p, h->d_st_snap.p, (size_t)h->frames * sizeof(PwppStateScalar), hipMemcpyDeviceToDevice, h->stream));
                    HIPCHK(hipMemcpyAsync(h->d_pl_stream.p, h->d_pl_snap.p, (size_t)h->frames * sizeof(PwppPlaneState), hipMemcpyDeviceToDevice, h->stream));
                    HIPCHK(hipMemcpyAsync(h->d_hist_stream.p, h->d_hist_snap.p, (size_t)h->frames * slab * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
                } else {
                    for (int f : redo) {
                        HIPCHK(hipMemcpyAsync(h->d_st_stream.p + f, h->d_st_snap.p + f, sizeof(PwppStateScalar), hipMemcpyDeviceToDevice, h->stream));
                        HIPCHK(hipMemcpyAsync(h->d_pl_stream.p + f, h->d_pl_snap.p + f, sizeof(PwppPlaneState), hipMemcpyDeviceToDevice, h->stream));
                        HIPCHK(hipMemcpyAsync(h->d_hist_stream.p + (size_t)f * slab, h->d_hist_snap.p + (size_t)f * slab, slab * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
                    }
                }
            }
            if (!in_place) {
                h->one_pass_redone_frames += h->frames;
                int rc = launch_prepared(h, false);
                if (rc) return rc;
                h->pending = true;
                if ((rc = finish_pending(h))) return rc;
                return read_observed(h);  // the exact counts of the redo size the next table
            }
            h->one_pass_redone_frames += (long long)redo.size();
            PwppBatch bt;
            fill_batch(h, bt);
            bt.cap_off = nullptr;  // compact layout, exact two-pass binning (K1, K2, K3)
            bt.next_slabs = 1;     // (the other copy of the counters was zeroed for a one-pass call by the first attempt's K5 already)
            for (size_t i = 0; i < redo.size();) {  // runs of neighbouring frames go through the pipeline together
                size_t j = i + 1;
                while (j < redo.size() && redo[j] == redo[j - 1] + 1) ++j;
                const int f0 = redo[i], nf = (int)(j - i);
                PwppBatch v = frame_range(h, bt, f0, nf);  // (no_clear set: the three counter slabs of a frame RANGE are not adjacent)
                int vmax = 0;
                for (int f = f0; f < f0 + nf; ++f) {
                    h->frame_two_pass[(size_t)f] = 1;
                    vmax = h->descs[(size_t)f].n > vmax ? h->descs[(size_t)f].n : vmax;
                }
                v.max_n = vmax;
                const size_t words = (size_t)nf * (size_t)NP * sizeof(uint32_t);
                HIPCHK(hipMemsetAsync(v.part_count, 0, words, h->stream));
                HIPCHK(hipMemsetAsync(v.part_off, 0, words, h->stream));
                HIPCHK(hipMemsetAsync(v.part_cursor, 0, words, h->stream));
                HIPCHK(hipMemsetAsync(v.results, 0, (size_t)nf * sizeof(PwppFrameResult), h->stream));
                if (const int rc = launch_pipeline(h, v, 7)) return rc;
                i = j;
            }
            HIPCHK(hipStreamSynchronize(h->stream));
            redone_in_place = true;
        }
    }
    // Frames with a patch whose first fit set was empty (pwpp_fit.hip: needs_previous_plane -- a lowest height of -inf or
    // beyond 1e15 m, num_lpr = 0; never a real scan): K5 / K6 left them alone; k_fit_fixup fits those patches in the
    // reference's order from the plane fitted before them, then K5 and K6 finish the frame.
    {
        bool any = false;
        for (int f = 0; f < h->frames; ++f) any = any || (h->h_results.p[f].overflow & 2) != 0;
        if (any) {
            PwppBatch bt;
            fill_batch(h, bt);
            bt.fixup_run = 1;
            for (int f = 0; f < h->frames; ++f) {
                if (!(h->h_results.p[f].overflow & 2)) continue;
                PwppBatch v = frame_range(h, bt, f, 1);
                v.cap_off = was_one_pass && !h->frame_two_pass[(size_t)f] ? h->d_cap_off.p : nullptr;  // (a frame redone in place is in the compact layout)
                if (v.cap_off) set_arena(h, v, f);  // (where its moved parts' bits live: pwpp_member_offset)
                if (const int rc = launch_pipeline(h, v, 2 | 4 | 8)) return rc;
                ++h->fixed_up_frames;
            }
            HIPCHK(hipStreamSynchronize(h->stream));
        }
    }
    for (int f = 0; f < h->frames; ++f) {
        if (h->h_results.p[f].overflow & 4) ++h->clamped_frames;
        if ((h->h_results.p[f].overflow & 8) && !(h->frame_two_pass.size() > (size_t)f && h->frame_two_pass[(size_t)f])) ++h->arena_frames;
    }
    h->have_results = true;
    if (redone_in_place) {  // the exact counts of the redone frames are in d_bin_max now: they size the next table
        const int rc = read_observed(h);
        if (rc) return rc;
    } else if (was_one_pass) {
        // a part that held more points than the table was built for (it ate into its head-room, or was moved into the arena): size
        // the table anew before the next batch
        h->observed.assign(h->h_bin_max.p, h->h_bin_max.p + h->cap_table.size());
        for (size_t b = 0; b < h->cap_table.size() && !h->table_stale; ++b)
            if (h->observed[b] > (b < h->cap_seen.size() ? h->cap_seen[b] : 0u) && h->cap_table[b] > 0u) h->table_stale = true;
    }
    if (h->mode == PWPP_MODE_STREAMS) h->hist_check_due = true;
    return defer_tail ? PWPP_OK : settle_k5_tail(h);
}

// What every entry point that works on a handle starts with: the handle, its device, and the call in flight landed
// (lists_only: see finish_pending).
int enter(pwpp_handle *h, bool lists_only = false) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    const int rc = use_device(h);
    return rc ? rc : finish_pending(h, lists_only);
}

int check_frame(pwpp_handle *h, int frame) {
    const int rc = enter(h, true);  // (a call's results: counts, lists, patch rows)
    if (rc) return rc;
    if (!h->have_results) return fail(PWPP_E_STATE, "no frame has been processed yet");
    if (frame < 0 || frame >= h->frames) return fail(PWPP_E_ARG, "frame %d out of range [0,%d)", frame, h->frames);
    return PWPP_OK;
}

// a frame of the last call's results, and the per-point output `which` among them
int need_output(pwpp_handle *h, int frame, Output which) {
    const int rc = check_frame(h, frame);
    if (rc) return rc;
    if (!(h->outputs_last & bit(which))) return fail(PWPP_E_STATE, "%s", kOutputMissing[which]);
    return PWPP_OK;
}

// One frame's span of a per-point array of the output `which` (`elem` bytes per point, laid out like d_out), or the whole batch.
int copy_output(pwpp_handle *h, Output which, int frame, bool whole_batch, void *out, const void *src_all, size_t elem) {
    const int rc = need_output(h, frame, which);
    if (rc) return rc;
    const int64_t first = whole_batch ? 0 : h->h_base.p[frame], end = h->h_base.p[whole_batch ? h->frames : frame + 1];
    if (end > first) {
        if (!out) return fail(PWPP_E_ARG, "null output");
        HIPCHK(hipMemcpyAsync(out, static_cast<const char *>(src_all) + (size_t)first * elem, (size_t)(end - first) * elem, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return PWPP_OK;
}

// One call's arrays in a staging buffer of the handle, for both memory kinds.  The call declares its sections in buffer order:
// 4-byte words, the caller's pointer (null: an optional array that is absent -- a null device pointer, no copy; it keeps the room
// of its words, so a call declares it with 0 words where none is wanted) and what becomes of it.  PWPP_MEM_DEVICE: the kernels work
// on the caller's pointers, only the kKept sections lie in the buffer, end() notes the enqueued work.  PWPP_MEM_HOST: every section
// lies in the buffer, begin() uploads the kIn ones, end() downloads the kOut ones and waits.  A table the call built on the host for
// its kernels (add_upload): begin() hands the words to the handle, which owns them until the next call that uploads (the caller's arrays
// may go on return), and enqueues their copy -- pageable memory, nothing waits.  `align`: every section starts at a multiple of so many words.
class Staging {
  public:
    enum Dir { kIn, kOut, kKept, kUpload };  // read by the kernels | written by them | theirs alone | built for them: these two in the buffer whatever the memory kind
    Staging(pwpp_handle *h, DevBuf<uint32_t> &buf, int mem, size_t align = 1) : h_(h), buf_(buf), host_(mem == PWPP_MEM_HOST), align_(align) {}
    // (`bytes`: of the caller's array where it is no whole number of words -- a byte image; a section beyond kMaxSections is counted, not stored: begin() refuses the call)
    int add(size_t words, const void *user, Dir dir, size_t bytes = 0) {
        if (n_ < kMaxSections) sec_[n_] = Section{words_, words, bytes ? bytes : words * 4, user, dir};
        if (dir == kKept || dir == kUpload || host_) words_ += (words + align_ - 1) / align_ * align_;
        return n_++;
    }
    // A byte image of `bytes` bytes (occupancy, cost, a class per cell): whole words in the buffer, the bytes copied.  An optional one that is absent --
    // no pointer, and not kKept -- declares 0 words like any absent array.
    int add_bytes(size_t bytes, const void *user, Dir dir) {
        const bool present = user || dir == kKept;
        return add(present ? (bytes + 3) / 4 : 0, user, dir, present ? bytes : 0);
    }
    int add_upload(std::vector<uint32_t> &&words) {  // (a vector's words stay where they are when it moves)
        up_.push_back(std::move(words));
        return add(up_.back().size(), up_.back().data(), kUpload);
    }
    int begin() {
        if (n_ > kMaxSections) return fail(PWPP_E_STATE, "the call declares %d staged sections: at most %d are supported", n_, kMaxSections);
        const int rc = buf_.ensure(words_);
        if (rc) return rc;
        if (!up_.empty()) h_->uploads.swap(up_);  // (those of the last call that uploaded end with this object)
        for (int k = 0; k < n_; ++k)
            if ((sec_[k].dir == kUpload || (host_ && sec_[k].dir == kIn)) && sec_[k].user && sec_[k].words > 0)
                HIPCHK(hipMemcpyAsync(buf_.p + sec_[k].at, sec_[k].user, sec_[k].bytes, hipMemcpyHostToDevice, h_->stream));
        return PWPP_OK;
    }
    template <class T>
    T *dev(int k) const {  // (after begin(): the buffer may have moved)
        const Section &c = sec_[k];
        if (c.dir != kKept && c.dir != kUpload && (!host_ || !c.user)) return static_cast<T *>(const_cast<void *>(c.user));
        return reinterpret_cast<T *>(buf_.p + c.at);
    }
    int end() {
        if (!host_) {
            h_->ground_query_queued = true;
            return PWPP_OK;
        }
        for (int k = 0; k < n_; ++k)
            if (sec_[k].dir == kOut && sec_[k].user && sec_[k].words > 0)
                HIPCHK(hipMemcpyAsync(const_cast<void *>(sec_[k].user), buf_.p + sec_[k].at, sec_[k].bytes, hipMemcpyDeviceToHost, h_->stream));
        HIPCHK(hipStreamSynchronize(h_->stream));
        return PWPP_OK;
    }

  private:
    static constexpr int kMaxSections = 20;  // (pwpp_track_obstacles declares 17: the labelling's and the association's)
    struct Section {
        size_t at, words, bytes;
        const void *user;  // (kUpload: the words, in up_ and after begin() in the handle)
        Dir dir;
    };
    pwpp_handle *h_;
    DevBuf<uint32_t> &buf_;
    const bool host_;
    const size_t align_;
    size_t words_ = 0;
    int n_ = 0;
    std::vector<std::vector<uint32_t>> up_;
    Section sec_[kMaxSections];
};
constexpr size_t kClusterAlign = 4;  // the cluster buffer's sections start at multiples of 16 bytes (the table's 64-bit sums need 8)

int set_output(pwpp_handle *h, Output which, int on) {
    const int rc = enter(h);
    if (rc) return rc;
    h->outputs = on ? h->outputs | bit(which) : h->outputs & ~bit(which);
    return PWPP_OK;
}

// The options that pick a kernel variant, 0 .. max: what a value means stands at the handle's member.
struct PathOption {
    const char *name;
    int pwpp_handle::*member;
    int max;
};
constexpr PathOption kPathOptions[] = {
    {"records_path", &pwpp_handle::records_path, 2},
    {"clusters_path", &pwpp_handle::clusters_path, 1},
    {"distance_path", &pwpp_handle::distance_path, 1},
    {"visibility_path", &pwpp_handle::visibility_path, 1},
    {"viewshed_path", &pwpp_handle::viewshed_path, 2},
    {"beams_path", &pwpp_handle::beams_path, 2},
    {"fusion_path", &pwpp_handle::fusion_path, 1},
    {"elevation_path", &pwpp_handle::elevation_path, 2},
    {"terrain_path", &pwpp_handle::terrain_path, 2},
    {"reach_path", &pwpp_handle::reach_path, 2},
    {"route_path", &pwpp_handle::route_path, 2},
    {"footprint_path", &pwpp_handle::footprint_path, 2},
    {"costmap_path", &pwpp_handle::costmap_path, 2},
    {"match_path", &pwpp_handle::match_path, 2},
    {"evidence_path", &pwpp_handle::evidence_path, 2},
    {"boxes_path", &pwpp_handle::boxes_path, 2},
    {"hulls_path", &pwpp_handle::hulls_path, 2},
};
const PathOption *path_option(const std::string &name) {
    for (const PathOption &o : kPathOptions)
        if (name == o.name) return &o;
    return nullptr;
}

}  // namespace

extern "C" {

const char *pwpp_last_error(void) { return g_err.c_str(); }

int pwpp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *pwpp_kernel_name(int k) {
    if (k == 0 && g_slot0_one_pass) return "k_czm_bin_scatter";  // what the last launch ran in the first slot
    return (k >= 0 && k < PWPP_NUM_KERNELS) ? kKernelNames[k] : "";
}

int pwpp_params_default(pwpp_params *p) {  // reference patchworkpp.h:79-111
    if (!p) return fail(PWPP_E_ARG, "null params");
    std::memset(p, 0, sizeof(*p));
    p->verbose = 0;
    p->enable_RNR = 1;
    p->enable_RVPF = 1;
    p->enable_TGR = 1;
    p->num_iter = 3;
    p->num_lpr = 20;
    p->num_min_pts = 10;
    p->num_zones = 4;
    p->num_rings_of_interest = 4;
    p->RNR_ver_angle_thr = -15.0;
    p->RNR_intensity_thr = 0.2;
    p->sensor_height = 1.723;
    p->th_seeds = 0.125;
    p->th_dist = 0.125;
    p->th_seeds_v = 0.25;
    p->th_dist_v = 0.1;
    p->max_range = 80.0;
    p->min_range = 2.7;
    p->uprightness_thr = 0.707;
    p->adaptive_seed_selection_margin = -1.2;
    p->intensity_thr = 0.0;  // uninitialised in the reference (patchworkpp.h:67), never read
    const int sectors[4] = {16, 32, 54, 32}, rings[4] = {2, 4, 4, 4};
    for (int k = 0; k < 4; ++k) {
        p->num_sectors_each_zone[k] = sectors[k];
        p->num_rings_each_zone[k] = rings[k];
    }
    p->max_flatness_storage = 1000;
    p->max_elevation_storage = 1000;
    return PWPP_OK;
}

int pwpp_set_num_streams(pwpp_handle *h, int streams) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (streams < 1) return fail(PWPP_E_ARG, "streams must be >= 1");
    int rc = enter(h);
    if (rc) return rc;
    if ((rc = h->d_st_stream.ensure((size_t)streams))) return rc;
    if ((rc = h->d_hist_stream.ensure((size_t)streams * 8 * (size_t)h->stream_hist_cap))) return rc;
    if ((rc = h->d_pl_stream.ensure((size_t)streams))) return rc;
    HIPCHK(hipMemset(h->d_pl_stream.p, 0, (size_t)streams * sizeof(PwppPlaneState)));  // a new object's members
    std::vector<PwppStateScalar> init((size_t)streams);
    for (auto &s : init) fill_default_state(h, s);
    HIPCHK(hipMemcpy(h->d_st_stream.p, init.data(), init.size() * sizeof(PwppStateScalar), hipMemcpyHostToDevice));
    h->num_streams = streams;
    return PWPP_OK;
}

int pwpp_create(const pwpp_params *p, int device, pwpp_handle **out) {
    if (!p || !out) return fail(PWPP_E_ARG, "null argument");
    *out = nullptr;
    PwppDevParams dp;
    const int max_near_sectors = build_dev_params(*p, dp);
    if (max_near_sectors < 0) return max_near_sectors;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(PWPP_E_NODEVICE, "no HIP device available (%s); this library has no CPU path",
                    e != hipSuccess ? hipGetErrorString(e) : "0 devices");
    if (device < 0 || device >= ndev) return fail(PWPP_E_ARG, "device %d out of range [0,%d)", device, ndev);
    HIPCHK(hipSetDevice(device));
    std::vector<float2> origin;
    dp.fxp_wide = 1;  // contract v4 (option "exact_moments")
    if (const char *e = std::getenv("PWPP_EXACT_MOMENTS")) dp.fxp_wide = std::atoi(e) != 0;
    dp.fxp_zr = (float)fxp_geometry(dp, origin, dp.fxp_shift, dp.fxp_wide != 0);
    std::vector<float4> boxes;
    bin_boxes(dp, boxes);
    dp.hi_split = 0.6f;  // option "hi_split"
    dp.split_end = dp.bin_base[1];  // option "hi_split_zones": the zones whose bins are stored in two parts (default: the first)
    pwpp_handle *h = new pwpp_handle;
    h->params = *p;
    h->dp = dp;
    h->device = device;
    // The tuning / test switches: read once, here (not in the launch path), and said out loud.
    if (const char *e = std::getenv("PWPP_DEBUG_FLAGS")) h->debug_flags = std::atoi(e);
    if ((h->debug_flags & 4) && (h->debug_flags & 8)) {  // (the two sets of timing probes share one array: pwpp_set_option refuses the pair, the environment path says what it does)
        h->debug_flags &= ~8;
        std::fprintf(stderr, "pwpp: PWPP_DEBUG_FLAGS has both timing-probe sets (4 and 8), which share one array: 8 dropped\n");
    }
    if (const char *e = std::getenv("PWPP_FIT_PLAN")) h->fit_plan = e;
    h->no_one_pass = std::getenv("PWPP_NO_ONE_PASS") != nullptr;
    if (const char *e = std::getenv("PWPP_ONE_PASS_MIN_FRAMES")) h->one_pass_min_frames = h->one_pass_min_fresh = std::atoi(e);
    if (const char *e = std::getenv("PWPP_OVERLAP_RANGES")) h->overlap_ranges = std::atoi(e) < 2 ? 2 : std::atoi(e);
    if (const char *e = std::getenv("PWPP_FIT_STREAMS")) h->num_fit_streams = std::atoi(e) < 1 ? 1 : (std::atoi(e) > 8 ? 8 : std::atoi(e));
    if (const char *e = std::getenv("PWPP_HI_SPLIT")) h->dp.hi_split = (float)std::atof(e);
    if (const char *e = std::getenv("PWPP_HI_SPLIT_ZONES")) h->dp.split_end = h->dp.bin_base[std::atoi(e) < 0 ? 0 : (std::atoi(e) > 4 ? 4 : std::atoi(e))];
    if (const char *e = std::getenv("PWPP_ONE_PASS_SCALE")) {
        const double v = std::atof(e);
        if (v > 0.0 && v <= 1024.0) h->one_pass_scale = v;
        else std::fprintf(stderr, "pwpp: ignoring PWPP_ONE_PASS_SCALE=%s (a positive number up to 1024 expected)\n", e);
    }
    if (std::getenv("PWPP_EXACT_MOMENTS")) std::fprintf(stderr, "pwpp: exact_moments=%d taken from the environment (PWPP_EXACT_MOMENTS)\n", h->dp.fxp_wide);
    if (h->debug_flags || !h->fit_plan.empty() || h->no_one_pass || std::getenv("PWPP_ONE_PASS_MIN_FRAMES") ||
        std::getenv("PWPP_ONE_PASS_SCALE") || std::getenv("PWPP_OVERLAP") || std::getenv("PWPP_OVERLAP_RANGES") || std::getenv("PWPP_HI_SPLIT") ||
        std::getenv("PWPP_HI_SPLIT_ZONES"))
        std::fprintf(stderr, "pwpp: tuning options taken from the environment (PWPP_*): debug_flags=%d fit_plan='%s' "
                             "no_one_pass=%d one_pass_min_frames=%d one_pass_scale=%g overlap=%d hi_split=%g (first %d bins)\n", h->debug_flags,
                     h->fit_plan.c_str(), (int)h->no_one_pass, h->one_pass_min_frames, h->one_pass_scale,
                     std::getenv("PWPP_OVERLAP") ? std::atoi(std::getenv("PWPP_OVERLAP")) : 1, (double)h->dp.hi_split, h->dp.split_end);
    const int storage = p->max_elevation_storage > p->max_flatness_storage ? p->max_elevation_storage : p->max_flatness_storage;
    h->stream_hist_cap = (storage + max_near_sectors + 1024 + 1) & ~1;  // (even: k_gle_tgr fetches the histories two entries at a time)
    h->max_pushes_per_frame = max_near_sectors;
    h->fresh_hist_cap = (max_near_sectors + 2 + 1) & ~1;
    if (const char *e = std::getenv("PWPP_OVERLAP")) h->overlap = std::atoi(e) != 0;  // (pwpp_set_overlap; PWPP_OVERLAP=0 runs existing programs on one stream)
    hipError_t se = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (se == hipSuccess) se = hipStreamCreateWithFlags(&h->aux_stream, hipStreamNonBlocking);
    // The streams of the overlap schedule are created HERE, together (round 5): the HIP runtime deals streams to its four hardware
    // queues in creation order, and a fit stream created lazily -- after some other handle's streams -- could land on the queue of
    // this handle's own memory stream: the two then run one after the other (3.18 instead of 2.6 ms per 1024-frame step,
    // tools/sync_after_pipelined.py).
    for (int k = 1; se == hipSuccess && k < h->num_fit_streams; ++k) {
        hipStream_t st = nullptr;
        se = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
        if (se == hipSuccess) h->extra_streams.push_back(st);
    }
    if (se == hipSuccess) se = hipEventCreateWithFlags(&h->aux_fork, hipEventDisableTiming);
    if (se == hipSuccess) se = hipEventCreateWithFlags(&h->aux_join, hipEventDisableTiming);
    if (se == hipSuccess) se = hipEventCreate(&h->ev_begin);
    if (se == hipSuccess) se = hipEventCreate(&h->ev_end);
    for (int k = 0; k <= PWPP_NUM_KERNELS && se == hipSuccess; ++k) se = hipEventCreate(&h->ev_k[k]);
    if (se != hipSuccess) {
        pwpp_destroy(h);
        return fail(PWPP_E_HIP, "stream/event creation failed: %s", hipGetErrorString(se));
    }
    int rc = pwpp_set_num_streams(h, 1);
    const size_t NP = (size_t)PWPP_NUM_PARTS(dp.num_bins);
    if (!rc) rc = h->h_bin_max.ensure(NP);
    if (!rc) rc = h->d_bin_max.ensure(NP);
    if (!rc && hipMemset(h->d_bin_max.p, 0, NP * sizeof(uint32_t)) != hipSuccess) rc = fail(PWPP_E_HIP, "hipMemset failed");
    if (!rc) rc = h->d_bin_bbox.ensure(boxes.size());
    if (!rc && hipMemcpy(h->d_bin_bbox.p, boxes.data(), boxes.size() * sizeof(float4), hipMemcpyHostToDevice) != hipSuccess)
        rc = fail(PWPP_E_HIP, "uploading the bin boxes failed");
    if (!rc) rc = h->d_bin_origin.ensure(origin.size());
    if (!rc && hipMemcpy(h->d_bin_origin.p, origin.data(), origin.size() * sizeof(float2), hipMemcpyHostToDevice) != hipSuccess)
        rc = fail(PWPP_E_HIP, "uploading the bin origins failed");
    if (rc) {
        pwpp_destroy(h);
        return rc;
    }
    if (p->verbose) std::printf("PatchWorkpp::PatchWorkpp() - INITIALIZATION COMPLETE (MI355X/HIP, %d CZM bins, fxp shift %d)\n", dp.num_bins, dp.fxp_shift);
    *out = h;
    return PWPP_OK;
}

int pwpp_destroy(pwpp_handle *h) {
    if (!h) return PWPP_OK;
    (void)hipSetDevice(h->device);
    sync_all_streams(h);
    for (BufBase *b : h->bufs) b->release();
    if (h->ev_begin) (void)hipEventDestroy(h->ev_begin);
    if (h->ev_end) (void)hipEventDestroy(h->ev_end);
    for (int k = 0; k <= PWPP_NUM_KERNELS; ++k)
        if (h->ev_k[k]) (void)hipEventDestroy(h->ev_k[k]);
    for (hipEvent_t e : h->ev_ranges) (void)hipEventDestroy(e);
    for (hipStream_t st : h->extra_streams) (void)hipStreamDestroy(st);
    if (h->aux_fork) (void)hipEventDestroy(h->aux_fork);
    if (h->aux_join) (void)hipEventDestroy(h->aux_join);
    if (h->aux_stream) (void)hipStreamDestroy(h->aux_stream);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return PWPP_OK;
}

}  // extern "C"

namespace {
struct FieldSpec {  // PWPP_LAYOUT_FIELDS: where the float32 fields of a point lie
    int step, off[4];
};
int estimate_batch(pwpp_handle *h, const float *const *points, const int32_t *n, int frames, int cols, int layout, int mem, int mode,
                   const FieldSpec *fs);
}  // namespace

extern "C" {

int pwpp_estimate_ground_batch(pwpp_handle *h, const float *const *points, const int32_t *n, int frames, int cols,
                               int layout, int mem, int mode) {
    if (layout != PWPP_LAYOUT_ROW_MAJOR && layout != PWPP_LAYOUT_COL_MAJOR) return fail(PWPP_E_ARG, "bad layout %d", layout);
    return estimate_batch(h, points, n, frames, cols, layout, mem, mode, nullptr);
}

int pwpp_estimate_ground_fields_batch(pwpp_handle *h, const void *const *data, const int32_t *n, int frames, int point_step,
                                      int off_x, int off_y, int off_z, int off_intensity, int mem, int mode) {
    if (point_step < 12 || (point_step & 3)) return fail(PWPP_E_ARG, "point_step=%d: a multiple of 4, at least 12, expected", point_step);
    const int off[4] = {off_x, off_y, off_z, off_intensity};
    for (int k = 0; k < 4; ++k) {
        if (k == 3 && off[k] < 0) continue;  // no intensity field: RNR is skipped, as for an N x 3 matrix (patchworkpp.cpp:379-382)
        if (off[k] < 0 || (off[k] & 3) || off[k] + 4 > point_step)
            return fail(PWPP_E_ARG, "field offset %d does not name a 4-byte aligned float32 inside a point of %d bytes", off[k], point_step);
    }
    // the fields are read in place as float32 (host: merged copies computed in units of floats; device: aligned loads): a
    // blob that does not start on a 4-byte boundary cannot be read that way
    if (!data || !n) return fail(PWPP_E_ARG, "null argument");  // (the handle is checked by estimate_batch: the alignment check needs none)
    if (frames < 1 || frames > 65535) return fail(PWPP_E_ARG, "frames=%d: 1 ... 65535 per call expected", frames);  // (before n[] / data[] are walked)
    for (int i = 0; i < frames; ++i)
        if (n[i] > 0 && (reinterpret_cast<uintptr_t>(data[i]) & 3u) != 0)
            return fail(PWPP_E_ARG, "frame %d: data pointer %p is not 4-byte aligned", i, data[i]);
    FieldSpec fs;
    fs.step = point_step;
    for (int k = 0; k < 4; ++k) fs.off[k] = off[k] < 0 ? -1 : off[k];
    return estimate_batch(h, reinterpret_cast<const float *const *>(data), n, frames, off_intensity >= 0 ? 4 : 3, PWPP_LAYOUT_FIELDS, mem, mode, &fs);
}

int pwpp_estimate_ground_fields(pwpp_handle *h, const void *data, int n, int point_step, int off_x, int off_y, int off_z, int off_intensity) {
    const void *ptrs[1] = {data};
    const int32_t ns[1] = {n};
    return pwpp_estimate_ground_fields_batch(h, ptrs, ns, 1, point_step, off_x, off_y, off_z, off_intensity, PWPP_MEM_HOST, PWPP_MODE_STREAMS);
}

}  // extern "C"

namespace {
int estimate_batch(pwpp_handle *h, const float *const *points, const int32_t *n, int frames, int cols, int layout, int mem, int mode,
                   const FieldSpec *fs) {
    if (!h || !points || !n) return fail(PWPP_E_ARG, "null argument");
    if (frames < 1) return fail(PWPP_E_ARG, "frames must be >= 1");
    if (frames > 65535) return fail(PWPP_E_ARG, "%d frames: at most 65535 per call (the frame is a grid dimension of the kernels)", frames);
    if (cols != 3 && cols != 4) return fail(PWPP_E_ARG, "cols=%d: 3 or 4 expected", cols);
    const int64_t floats_per_point = fs ? fs->step / 4 : cols;  // what a frame occupies in the staging buffer
    if (mem != PWPP_MEM_HOST && mem != PWPP_MEM_DEVICE && mem != PWPP_MEM_HOST_PINNED) return fail(PWPP_E_ARG, "bad mem %d", mem);
    const bool from_host = mem != PWPP_MEM_DEVICE;
    if (mode != PWPP_MODE_FRESH && mode != PWPP_MODE_STREAMS) return fail(PWPP_E_ARG, "bad mode %d", mode);
    int rc = enter(h);
    if (rc) return rc;
    if (mode == PWPP_MODE_STREAMS && frames > h->num_streams)
        return fail(PWPP_E_ARG, "%d frames but only %d streams (pwpp_set_num_streams)", frames, h->num_streams);
    const size_t xf_count = h->input_xf.size() / 12;
    if (xf_count > 1 && xf_count != (size_t)frames)  // (before anything of the last call is touched: its results stay readable)
        return fail(PWPP_E_ARG, "%d frames but %zu input transforms (pwpp_set_input_transforms: one, or one per frame)", frames, xf_count);

    const int B = h->dp.num_bins, NB = B + 2, NP = PWPP_NUM_PARTS(B);
    int64_t total = 0, total_in = 0;
    int max_n = 0;
    for (int f = 0; f < frames; ++f) {
        if (n[f] < 0 || n[f] > (1 << 22)) return fail(PWPP_E_ARG, "frame %d: %d points (0..4194304 supported)", f, n[f]);
        if (n[f] > 0 && !points[f]) return fail(PWPP_E_ARG, "frame %d: null points", f);
        if (mem == PWPP_MEM_DEVICE && layout == PWPP_LAYOUT_ROW_MAJOR && cols == 4 && ((uintptr_t)points[f] & 15u))
            return fail(PWPP_E_ARG, "frame %d: device buffer must be 16-byte aligned", f);
        total += n[f];
        total_in += ((int64_t)n[f] * floats_per_point + 3) & ~(int64_t)3;
        if (n[f] > max_n) max_n = n[f];
    }
    if (total >= ((int64_t)1 << 31)) return fail(PWPP_E_ARG, "batch of %lld points exceeds 2^31", (long long)total);
    const size_t tp = (size_t)(total > 0 ? total : 1);

    // ---- 1. everything but the bin-ordered buffers
    if ((rc = h->d_frames.ensure((size_t)frames))) return rc;
    if ((rc = h->h_frames.ensure((size_t)frames))) return rc;
    if ((rc = h->h_base.ensure((size_t)frames + 1))) return rc;
    // (the per-point codes are the two-pass path's: a one-pass batch only needs them for its histogram probe and for a frame that is
    // binned again -- allocated there, 2 bytes per point less to hold otherwise)
    if ((rc = h->d_out.ensure(tp))) return rc;
    if (h->output_order == PWPP_ORDER_REFERENCE) {
        if ((rc = h->d_ord_a.ensure(tp))) return rc;
        if ((rc = h->d_ord_b.ensure(tp))) return rc;
        if ((rc = h->d_ord_work.ensure((size_t)frames * (size_t)(1 + 2 * NB)))) return rc;
    }
    if (labels_on(h)) {  // (16 bytes of slack: the label kernels read whole 16-byte pieces)
        if ((rc = h->d_labels.ensure(tp + 16))) return rc;
        if (h->output_order == PWPP_ORDER_CLOUD && (rc = h->d_label_tiles.ensure((size_t)frames * (size_t)label_tile_stride(max_n)))) return rc;
    }
    if (h->outputs & bit(kPointPlanes)) {
        if ((rc = h->d_pt_patch.ensure(tp))) return rc;
        if ((rc = h->d_pt_dist.ensure(tp))) return rc;
        if ((rc = h->d_pt_rows.ensure((size_t)frames * B))) return rc;
    }
    h->record_bytes = fs ? fs->step : 4 * cols;
    if ((h->outputs & bit(kPointRecords)) && (rc = h->d_records.ensure(tp * (size_t)h->record_bytes + 64))) return rc;  // (64 bytes of slack behind the last row)
    h->outputs_last = outputs_on(h);
    if ((rc = h->d_bins.ensure((size_t)frames * NB * 4))) return rc;
    if ((rc = h->d_parts.ensure(2 * counters_copy_words((size_t)frames * NP)))) return rc;  // two copies
    if ((rc = h->d_recs.ensure((size_t)frames * B))) return rc;
    if ((rc = h->d_cls_start.ensure((size_t)frames * PWPP_CLS_STRIDE))) return rc;
    if ((rc = h->d_cls_list.ensure((size_t)frames * B))) return rc;
    if ((rc = h->d_centers.ensure((size_t)frames * B * 3))) return rc;
    if ((rc = h->d_normals.ensure((size_t)frames * B * 3))) return rc;
    if ((rc = h->d_results.ensure(2 * (size_t)frames))) return rc;  // two copies
    if ((rc = h->d_dbg.ensure(64))) return rc;
    if ((rc = h->h_results.ensure((size_t)frames))) return rc;
    if (mode == PWPP_MODE_FRESH) {
        if ((rc = h->d_st_fresh.ensure((size_t)frames))) return rc;
        if ((rc = h->d_hist_fresh.ensure((size_t)frames * 8 * (size_t)h->fresh_hist_cap))) return rc;
        if ((rc = h->d_pl_fresh.ensure((size_t)frames))) return rc;
    }
    if (from_host && (rc = h->d_in.ensure((size_t)(total_in > 0 ? total_in : 4)))) return rc;
    if (xf_count) {  // the transforms this call runs with, on the device before its first kernel; copied only when they changed
        const size_t floats = h->input_xf.size();
        if (h->d_xf.cap < floats) h->xf_on_device = 0;
        if ((rc = h->d_xf.ensure(floats))) return rc;
        if ((rc = h->h_xf.ensure(floats))) return rc;
        if (h->xf_on_device != floats || std::memcmp(h->h_xf.p, h->input_xf.data(), floats * sizeof(float)) != 0) {
            std::memcpy(h->h_xf.p, h->input_xf.data(), floats * sizeof(float));
            HIPCHK(hipMemcpyAsync(h->d_xf.p, h->h_xf.p, floats * sizeof(float), hipMemcpyHostToDevice, h->stream));
            h->xf_on_device = floats;
        }
    }

    // ---- 2. frame descriptors; host inputs start their way to the device
    h->descs.resize((size_t)frames);
    int64_t base = 0, in_off = 0;
    const float *run_src = nullptr;  // pending host-to-device copy (merged run of adjacent frames)
    float *run_dst = nullptr;
    int64_t run_len = 0;
    for (int f = 0; f < frames; ++f) {
        PwppFrameDesc &d = h->descs[(size_t)f];
        std::memset(&d, 0, sizeof(d));
        d.n = n[f];
        d.cols = cols;
        d.layout = layout;
        if (fs) {
            d.step = fs->step;
            for (int k = 0; k < 4; ++k) d.off[k] = fs->off[k];
        }
        if (xf_count) d.xf = h->d_xf.p + 12 * (xf_count == 1 ? 0 : (size_t)f);
        d.base = base;
        if (mode == PWPP_MODE_FRESH) {
            d.state_in = -1;
            d.state_out = f;
        } else {
            d.state_in = f;
            d.state_out = f;
        }
        if (from_host) {
            d.pts = h->d_in.p + in_off;
            // Frames that lie back to back in host memory (one slab per chunk) go over in copies of up to
            // 32 MB: 2 MB copies reach 34 GB/s on this PCIe Gen5 x16 link, 8-32 MB ones 49-52 GB/s.
            const int64_t fl = (int64_t)n[f] * floats_per_point;
            if (fl > 0) {
                if (run_len > 0 && points[f] == run_src + run_len && h->d_in.p + in_off == run_dst + run_len &&
                    (run_len + fl) * (int64_t)sizeof(float) <= ((int64_t)32 << 20)) {
                    run_len += fl;
                } else {
                    if (run_len > 0) HIPCHK(hipMemcpyAsync(run_dst, run_src, (size_t)run_len * sizeof(float), hipMemcpyHostToDevice, h->stream));
                    run_src = points[f];
                    run_dst = h->d_in.p + in_off;
                    run_len = fl;
                }
            }
            in_off += (fl + 3) & ~(int64_t)3;
        } else {
            d.pts = points[f];
        }
        h->h_base.p[f] = base;
        base += n[f];
    }
    h->h_base.p[frames] = base;
    if (run_len > 0) HIPCHK(hipMemcpyAsync(run_dst, run_src, (size_t)run_len * sizeof(float), hipMemcpyHostToDevice, h->stream));
    h->frames = frames;
    h->mode = mode;

    // ---- 3. One-pass binning (fixed bin segments, k_czm_bin_scatter) for batches of independent frames: the
    // bin-ordered buffers hold frames x slots_per_frame records instead of one per point.  Used when the memory
    // is there; any overflow is caught when the batch lands and the batch is redone exactly.
    bool one_pass = false;
    const size_t compact_slots = tp + (size_t)frames * (size_t)((PWPP_SLOT_ALIGN - 1) * NP + PWPP_SLOT_ALIGN);  // parts padded to multiples of PWPP_SLOT_ALIGN slots
    size_t bin_slots = compact_slots;
    if (h->one_pass_holdoff > 0) {
        --h->one_pass_holdoff;
    } else if (!h->no_one_pass && frames >= (mode == PWPP_MODE_FRESH ? h->one_pass_min_fresh : h->one_pass_min_frames) && max_n > 0) {
        if (2 * (int64_t)max_n < h->cap_max_n) {  // a much smaller sensor than the table was built for: start over
            HIPCHK(hipMemsetAsync(h->d_bin_max.p, 0, (size_t)NP * sizeof(uint32_t), h->stream));
            h->have_observation = false;
        }
        if (!h->have_observation) {
            if ((rc = h->d_codes.ensure(tp))) return rc;
            if ((rc = probe_histogram(h))) return rc;
            h->table_stale = true;
        }
        if (h->table_stale || max_n > h->cap_max_n || 2 * (int64_t)max_n < h->cap_max_n || h->cap_few != (frames <= 16 && h->one_pass_scale >= 1.0))
            if ((rc = build_capacity_table(h, max_n + max_n / 8))) return rc;
        const size_t want = (size_t)frames * (size_t)h->slots_per_frame;
        size_t free_b = 0, total_b = 0;
        const size_t per_slot = 3 * sizeof(float) + sizeof(int32_t) + 1;  // z, {x, y}, cloud index (+ the slot's bit and its share of the pads in the membership plane)
        const size_t held = (h->d_sorted_z.cap + h->d_sorted_idx.cap) * sizeof(int32_t) + h->d_sorted_xy.cap * sizeof(float2) + h->d_member.cap;
        const bool have = h->d_sorted_z.cap >= want + 1024 && h->d_sorted_xy.cap >= want + 1024 && h->d_sorted_idx.cap >= want;  // already allocated
        if (have || (hipMemGetInfo(&free_b, &total_b) == hipSuccess && (want + want / 8 + 64) * per_slot * 21 / 20 <= free_b + held &&
                     want < ((size_t)1 << 40))) {
            one_pass = true;
            bin_slots = want > compact_slots ? want : compact_slots;  // (a redo after an overflow uses the compact layout)
        }
    }

    // ---- 4. the bin-ordered buffers (slack: the fit kernels fetch whole chunks, up to 512 points beyond a patch's end)
    const size_t member_pads = (size_t)frames * (size_t)NP * 2 * PWPP_MEMBER_PAD + 4096;
    if (one_pass && (h->d_sorted_z.ensure(bin_slots + 1024) || h->d_sorted_xy.ensure(bin_slots + 1024) || h->d_sorted_idx.ensure(bin_slots) ||
                     h->d_member.ensure(bin_slots / 8 + member_pads))) {  // (the membership plane is part of the trial, not a hard error after it)
        one_pass = false;  // the big allocation failed after all (fragmentation): compact layout, two-pass binning
        bin_slots = compact_slots;
        (void)hipGetLastError();
    }
    if ((rc = h->d_sorted_z.ensure(bin_slots + 1024))) return rc;
    if ((rc = h->d_sorted_xy.ensure(bin_slots + 1024))) return rc;
    if ((rc = h->d_sorted_idx.ensure(bin_slots))) return rc;
    if ((rc = h->d_member.ensure(bin_slots / 8 + member_pads))) return rc;
    if (one_pass) {
        h->d_codes.release();  // (a cold handle's probe needed them; a redo gets them back: finish_pending)
    } else if ((rc = h->d_codes.ensure(tp))) {
        return rc;
    }
    if (one_pass && h->arena_slots && (rc = h->d_arena_tag.ensure((size_t)frames * h->arena_spill))) return rc;

    h->frames = frames;
    h->mode = mode;
    h->max_n = max_n;
    h->total_points = total;
    h->cols = cols;
    h->layout = layout;
    if (one_pass) {
        ++h->one_pass_batches;
        h->one_pass_frames += frames;
    }
    h->frame_two_pass.clear();
    if (one_pass && mode == PWPP_MODE_STREAMS) {  // stream i = frame i: keep what a redo must start from
        const size_t slab = (size_t)8 * (size_t)h->stream_hist_cap;
        if ((rc = h->d_st_snap.ensure((size_t)frames))) return rc;
        if ((rc = h->d_hist_snap.ensure((size_t)frames * slab))) return rc;
        if ((rc = h->d_pl_snap.ensure((size_t)frames))) return rc;
        // (the copies themselves are made by the binning kernel: PwppBatch.snap_*, set in launch_prepared)
    }
    if (frames > 64 && (rc = refresh_emit_long(h))) return rc;
    h->ground_rows_valid = false;  // (the ground queries rank this call's bins anew)
    if ((rc = launch_prepared(h, one_pass))) return rc;
    h->pending = true;
    h->have_results = false;
    if (mem == PWPP_MEM_HOST) return finish_pending(h);  // the caller's buffers may go away
    return PWPP_OK;
}
}  // namespace

extern "C" {

int pwpp_estimate_ground(pwpp_handle *h, const float *points, int n, int cols, int layout) {
    const float *ptrs[1] = {points};
    const int32_t ns[1] = {n};
    return pwpp_estimate_ground_batch(h, ptrs, ns, 1, cols, layout, PWPP_MEM_HOST, PWPP_MODE_STREAMS);
}

int pwpp_synchronize(pwpp_handle *h) {
    const int rc = enter(h, true);  // (the call's results; a stream's state is settled by whoever touches it: settle_k5_tail)
    if (rc) return rc;
    if (h->ground_query_queued) {  // (a PWPP_MEM_DEVICE ground query behind a call that had landed already)
        HIPCHK(hipStreamSynchronize(h->stream));
        h->ground_query_queued = false;
    }
    return PWPP_OK;
}

int pwpp_get_counts(pwpp_handle *h, int frame, int32_t *n_ground, int32_t *n_nonground, int32_t *n_patches) {
    int rc = check_frame(h, frame);
    if (rc) return rc;
    const PwppFrameResult &r = h->h_results.p[frame];
    if (n_ground) *n_ground = r.n_ground;
    if (n_nonground) *n_nonground = r.n_nonground;
    if (n_patches) *n_patches = r.n_patches;
    return PWPP_OK;
}

static int copy_indices(pwpp_handle *h, int frame, int32_t *out, bool ground) {
    int rc = check_frame(h, frame);
    if (rc) return rc;
    const PwppFrameResult &r = h->h_results.p[frame];
    const int64_t base = h->h_base.p[frame];
    const int count = ground ? r.n_ground : r.n_nonground;
    if (count > 0) {
        if (!out) return fail(PWPP_E_ARG, "null output");
        HIPCHK(hipMemcpy(out, h->d_out.p + base + (ground ? 0 : r.n_ground), (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return PWPP_OK;
}
int pwpp_get_ground_indices(pwpp_handle *h, int frame, int32_t *out) { return copy_indices(h, frame, out, true); }
int pwpp_get_nonground_indices(pwpp_handle *h, int frame, int32_t *out) { return copy_indices(h, frame, out, false); }

static int copy_xyz(pwpp_handle *h, int frame, float *out, bool ground) {
    int rc = check_frame(h, frame);
    if (rc) return rc;
    const PwppFrameResult &r = h->h_results.p[frame];
    const int64_t base = h->h_base.p[frame];
    const int count = ground ? r.n_ground : r.n_nonground;
    if (count <= 0) return PWPP_OK;
    if (!out) return fail(PWPP_E_ARG, "null output");
    if ((rc = h->d_xyz.ensure((size_t)count * 3))) return rc;
    const int lrc = pwpp_launch_gather_xyz(&h->descs[(size_t)frame], h->d_out.p + base + (ground ? 0 : r.n_ground), count, h->d_xyz.p, h->stream);
    if (lrc != 0) return fail(PWPP_E_HIP, "gather launch failed: %s", hipGetErrorString((hipError_t)lrc));
    HIPCHK(hipMemcpyAsync(out, h->d_xyz.p, (size_t)count * 3 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return PWPP_OK;
}
int pwpp_get_ground_xyz(pwpp_handle *h, int frame, float *out) { return copy_xyz(h, frame, out, true); }
int pwpp_get_nonground_xyz(pwpp_handle *h, int frame, float *out) { return copy_xyz(h, frame, out, false); }

static int copy_patch_rows(pwpp_handle *h, int frame, float *out, const float *src_all) {
    int rc = check_frame(h, frame);
    if (rc) return rc;
    const int np = h->h_results.p[frame].n_patches;
    if (np <= 0) return PWPP_OK;
    if (!out) return fail(PWPP_E_ARG, "null output");
    HIPCHK(hipMemcpy(out, src_all + (size_t)frame * h->dp.num_bins * 3, (size_t)np * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return PWPP_OK;
}
int pwpp_get_centers(pwpp_handle *h, int frame, float *out) { return copy_patch_rows(h, frame, out, h ? h->d_centers.p : nullptr); }
int pwpp_get_normals(pwpp_handle *h, int frame, float *out) { return copy_patch_rows(h, frame, out, h ? h->d_normals.p : nullptr); }

int pwpp_get_patch_records(pwpp_handle *h, int frame, pwpp_patch_record *out, int capacity) {
    int rc = check_frame(h, frame);
    if (rc) return rc;
    const int B = h->dp.num_bins, NB = B + 2;
    std::vector<PwppPatchRec> recs((size_t)B);
    std::vector<uint32_t> cnt((size_t)NB);
    HIPCHK(hipMemcpy(recs.data(), h->d_recs.p + (size_t)frame * B, (size_t)B * sizeof(PwppPatchRec), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cnt.data(), h->d_bins.p + (size_t)frame * NB, (size_t)NB * sizeof(uint32_t), hipMemcpyDeviceToHost));
    int k = 0, concentric = 0;
    for (int zone = 0; zone < 4; ++zone)
        for (int ring = 0; ring < h->dp.rings[zone]; ++ring, ++concentric)
            for (int sector = 0; sector < h->dp.sectors[zone]; ++sector) {
                const int bin = h->dp.bin_base[zone] + ring * h->dp.sectors[zone] + sector;
                if ((uint64_t)cnt[(size_t)bin] < h->dp.min_pts) continue;
                if (k < capacity && out) {
                    const PwppPatchRec &r = recs[(size_t)bin];
                    pwpp_patch_record &o = out[k];
                    std::memset(&o, 0, sizeof(o));
                    o.bin = bin;
                    o.concentric_idx = concentric;
                    o.n_points = (int)cnt[(size_t)bin];
                    o.n_ground = r.n_ground;
                    o.n_nonground = r.n_nonground;
                    o.decision = r.decision;
                    o.rounds = (r.valid >> 8) & 0xff;
                    for (int i = 0; i < 3; ++i) {
                        o.mean[i] = r.mean[i];
                        o.normal[i] = r.normal[i];
                        o.sv[i] = r.sv[i];
                    }
                    o.d = r.d;
                }
                ++k;
            }
    return k;  // number of patches (>= 0)
}

double pwpp_get_height(pwpp_handle *h) {
    pwpp_state s;
    if (!h) return 0.0;
    if (use_device(h) || finish_pending(h)) return 0.0;
    if (hipMemcpy(&s, h->d_st_stream.p, sizeof(s), hipMemcpyDeviceToHost) != hipSuccess) return 0.0;
    return s.sensor_height;
}

double pwpp_get_time_us(pwpp_handle *h) {
    if (!h) return 0.0;
    if (use_device(h) || finish_pending(h, true)) return 0.0;
    return h->time_us;
}

int pwpp_get_state(pwpp_handle *h, int index, pwpp_state *out) {
    if (!h || !out) return fail(PWPP_E_ARG, "null argument");
    int rc = enter(h);
    if (rc) return rc;
    const bool fresh = h->have_results && h->mode == PWPP_MODE_FRESH;
    const int limit = fresh ? h->frames : h->num_streams;
    if (index < 0 || index >= limit) return fail(PWPP_E_ARG, "state index %d out of range [0,%d)", index, limit);
    const PwppStateScalar *src = (fresh ? h->d_st_fresh.p : h->d_st_stream.p) + index;
    HIPCHK(hipMemcpy(out, src, sizeof(pwpp_state), hipMemcpyDeviceToHost));
    return PWPP_OK;
}

int pwpp_get_history(pwpp_handle *h, int index, int which, int ring, double *out, int capacity) {
    pwpp_state s;
    int rc = pwpp_get_state(h, index, &s);
    if (rc) return rc;
    if (which < 0 || which > 1 || ring < 0 || ring > 3) return fail(PWPP_E_ARG, "bad history selector");
    const bool fresh = h->mode == PWPP_MODE_FRESH && h->have_results;
    const int cap = fresh ? h->fresh_hist_cap : h->stream_hist_cap;
    const double *base = (fresh ? h->d_hist_fresh.p : h->d_hist_stream.p) + ((size_t)index * 8 + (size_t)which * 4 + ring) * cap;
    const int len = which == 0 ? s.elevation_len[ring] : s.flatness_len[ring];
    const int ncopy = len < capacity ? len : capacity;
    if (ncopy > 0) {
        if (!out) return fail(PWPP_E_ARG, "null output");
        HIPCHK(hipMemcpy(out, base, (size_t)ncopy * sizeof(double), hipMemcpyDeviceToHost));
    }
    return len;
}

int pwpp_set_state(pwpp_handle *h, int stream, const pwpp_state *in) {
    if (!h || !in) return fail(PWPP_E_ARG, "null argument");
    int rc = enter(h);
    if (rc) return rc;
    if (stream < 0 || stream >= h->num_streams) return fail(PWPP_E_ARG, "stream %d out of range", stream);
    PwppStateScalar s;
    std::memcpy(&s, in, sizeof(s));
    for (int k = 0; k < 4; ++k) s.elev_len[k] = s.flat_len[k] = 0;
    HIPCHK(hipMemcpy(h->d_st_stream.p + stream, &s, sizeof(s), hipMemcpyHostToDevice));
    return PWPP_OK;
}

int pwpp_get_fxp_geometry(const pwpp_params *p, int *shift, float *out_xy, int capacity_bins) {
    if (!p) return fail(PWPP_E_ARG, "null params");
    PwppDevParams dp;
    const int rc = build_dev_params(*p, dp);
    if (rc < 0) return rc;
    std::vector<float2> origin;
    int s = 0;
    (void)fxp_geometry(dp, origin, s, true);
    if (shift) *shift = s;
    if (out_xy) {
        if (capacity_bins < dp.num_bins) return fail(PWPP_E_ARG, "room for %d bins, %d needed", capacity_bins, dp.num_bins);
        for (int b = 0; b < dp.num_bins; ++b) {
            out_xy[2 * b] = origin[(size_t)b].x;
            out_xy[2 * b + 1] = origin[(size_t)b].y;
        }
    }
    return dp.num_bins;
}

int pwpp_get_bin_boxes(const pwpp_params *p, float *out_boxes, int capacity_bins) {
    if (!p) return fail(PWPP_E_ARG, "null params");
    PwppDevParams dp;
    const int rc = build_dev_params(*p, dp);
    if (rc < 0) return rc;
    if (!out_boxes) return dp.num_bins;
    if (capacity_bins < dp.num_bins) return fail(PWPP_E_ARG, "room for %d bins, %d needed", capacity_bins, dp.num_bins);
    std::vector<float4> boxes;
    bin_boxes(dp, boxes);
    for (int b = 0; b < dp.num_bins; ++b) {
        out_boxes[4 * b] = boxes[(size_t)b].x;
        out_boxes[4 * b + 1] = boxes[(size_t)b].y;
        out_boxes[4 * b + 2] = boxes[(size_t)b].z;
        out_boxes[4 * b + 3] = boxes[(size_t)b].w;
    }
    return dp.num_bins;
}

int64_t pwpp_get_clamped_frames(pwpp_handle *h) {
    if (!h) return PWPP_E_ARG;
    if (use_device(h) || finish_pending(h)) return PWPP_E_HIP;
    return (int64_t)h->clamped_frames;
}

int64_t pwpp_get_fixed_up_frames(pwpp_handle *h) {
    if (!h) return PWPP_E_ARG;
    if (use_device(h) || finish_pending(h)) return PWPP_E_HIP;
    return (int64_t)h->fixed_up_frames;
}

int pwpp_get_plane_state(pwpp_handle *h, int index, float out[10]) {
    if (!h || !out) return fail(PWPP_E_ARG, "null argument");
    int rc = enter(h);
    if (rc) return rc;
    const bool fresh = h->have_results && h->mode == PWPP_MODE_FRESH;
    const int limit = fresh ? h->frames : h->num_streams;
    if (index < 0 || index >= limit) return fail(PWPP_E_ARG, "state index %d out of range [0,%d)", index, limit);
    PwppPlaneState ps;
    HIPCHK(hipMemcpy(&ps, (fresh ? h->d_pl_fresh.p : h->d_pl_stream.p) + index, sizeof(ps), hipMemcpyDeviceToHost));
    for (int i = 0; i < 3; ++i) {
        out[i] = ps.mean[i];
        out[3 + i] = ps.normal[i];
        out[6 + i] = ps.sv[i];
    }
    out[9] = (float)ps.d;  // (d is a float dot product widened to double in the reference, patchworkpp.cpp:74)
    return PWPP_OK;
}

int pwpp_set_plane_state(pwpp_handle *h, int stream, const float in[10]) {
    if (!h || !in) return fail(PWPP_E_ARG, "null argument");
    int rc = enter(h);
    if (rc) return rc;
    if (stream < 0 || stream >= h->num_streams) return fail(PWPP_E_ARG, "stream %d out of range", stream);
    PwppPlaneState ps;
    for (int i = 0; i < 3; ++i) {
        ps.mean[i] = in[i];
        ps.normal[i] = in[3 + i];
        ps.sv[i] = in[6 + i];
    }
    ps.pad_ = 0.0f;
    ps.d = (double)in[9];
    HIPCHK(hipMemcpy(h->d_pl_stream.p + stream, &ps, sizeof(ps), hipMemcpyHostToDevice));
    return PWPP_OK;
}

int pwpp_set_history(pwpp_handle *h, int stream, int which, int ring, const double *values, int count) {
    if (!h || (count > 0 && !values)) return fail(PWPP_E_ARG, "null argument");
    int rc = enter(h);
    if (rc) return rc;
    if (stream < 0 || stream >= h->num_streams) return fail(PWPP_E_ARG, "stream %d out of range", stream);
    if (which < 0 || which > 1 || ring < 0 || ring > 3) return fail(PWPP_E_ARG, "bad history selector");
    if (count < 0 || count > (1 << 24)) return fail(PWPP_E_ARG, "count %d out of range", count);
    // (count is NOT limited to max_*_storage: the reference only trims a history in update_elevation_thr / update_flatness_thr,
    // which stop at the first ring without data, so a sensor that sees no ground in ring 0 grows the others without bound --
    // test_histories_the_reference_never_trims restores exactly such a state)
    for (int i = 0; i < count; ++i)
        if (!(std::fabs(values[i]) <= DBL_MAX)) return fail(PWPP_E_ARG, "history value %d is not finite: the reference only ever pushes finite heights and flatness values", i);
    while (count + h->max_pushes_per_frame + 8 > h->stream_hist_cap)
        if ((rc = grow_stream_histories(h, 2 * h->stream_hist_cap))) return rc;
    double *dst = h->d_hist_stream.p + ((size_t)stream * 8 + (size_t)which * 4 + ring) * h->stream_hist_cap;
    if (count > 0) HIPCHK(hipMemcpy(dst, values, (size_t)count * sizeof(double), hipMemcpyHostToDevice));
    const size_t field = which == 0 ? offsetof(PwppStateScalar, elev_len) : offsetof(PwppStateScalar, flat_len);
    char *dlen = reinterpret_cast<char *>(h->d_st_stream.p + stream) + field + (size_t)ring * sizeof(int32_t);
    const int32_t c32 = count;
    HIPCHK(hipMemcpy(dlen, &c32, sizeof(int32_t), hipMemcpyHostToDevice));
    return PWPP_OK;
}

int pwpp_get_device_view(pwpp_handle *h, pwpp_device_view *out) {
    if (!h || !out) return fail(PWPP_E_ARG, "null argument");
    int rc = enter(h);
    if (rc) return rc;
    if (!h->have_results) return fail(PWPP_E_STATE, "no frame has been processed yet");
    out->indices = h->d_out.p;
    out->frame_base = h->h_base.p;
    out->counts = reinterpret_cast<const int32_t *>(h->h_results.p);
    out->frames = h->frames;
    out->pad_ = 0;
    return PWPP_OK;
}

int pwpp_host_alloc(void **out, uint64_t bytes) {
    if (!out) return fail(PWPP_E_ARG, "null argument");
    *out = nullptr;
    hipError_t e = hipHostMalloc(out, (size_t)(bytes ? bytes : 1), hipHostMallocDefault);
    if (e != hipSuccess) return fail(PWPP_E_NOMEM, "hipHostMalloc(%llu) failed: %s", (unsigned long long)bytes, hipGetErrorString(e));
    return PWPP_OK;
}
int pwpp_host_free(void *p) {
    if (p) HIPCHK(hipHostFree(p));
    return PWPP_OK;
}

int pwpp_get_all_indices(pwpp_handle *h, int32_t *out, int64_t *frame_base, int32_t *counts) {
    int rc = check_frame(h, 0);
    if (rc) return rc;
    if (!out) return fail(PWPP_E_ARG, "null output");
    const int64_t total = h->h_base.p[h->frames];
    if (total > 0) {
        HIPCHK(hipMemcpyAsync(out, h->d_out.p, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    if (frame_base) std::memcpy(frame_base, h->h_base.p, ((size_t)h->frames + 1) * sizeof(int64_t));
    if (counts) std::memcpy(counts, h->h_results.p, (size_t)h->frames * sizeof(PwppFrameResult));
    return PWPP_OK;
}

int pwpp_set_profiling(pwpp_handle *h, int enable) {
    int rc = enter(h);
    if (rc) return rc;
    h->profiling = enable != 0;
    return PWPP_OK;
}
int pwpp_get_kernel_profile(pwpp_handle *h, double *sum_ms, int64_t *launches) {
    int rc = enter(h);
    if (rc) return rc;
    for (int k = 0; k < PWPP_NUM_KERNELS; ++k) {
        if (sum_ms) sum_ms[k] = h->prof_ms[k];
        if (launches) launches[k] = h->prof_launches[k];
    }
    return PWPP_OK;
}
int pwpp_reset_kernel_profile(pwpp_handle *h) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    for (int k = 0; k < PWPP_NUM_KERNELS; ++k) {
        h->prof_ms[k] = 0.0;
        h->prof_launches[k] = 0;
    }
    return PWPP_OK;
}
int pwpp_get_fxp_shift(pwpp_handle *h) { return h ? h->dp.fxp_shift : PWPP_E_ARG; }

int pwpp_get_fxp_origins(pwpp_handle *h, float *out_xy, int capacity_bins) {
    if (!h) return fail(PWPP_E_ARG, "null argument");
    const int B = h->dp.num_bins;
    if (!out_xy) return B;  // size query
    if (capacity_bins < B) return fail(PWPP_E_ARG, "room for %d bins, %d needed", capacity_bins, B);
    int rc = use_device(h);
    if (rc) return rc;
    HIPCHK(hipMemcpy(out_xy, h->d_bin_origin.p, (size_t)B * sizeof(float2), hipMemcpyDeviceToHost));
    return B;
}

int pwpp_set_option(pwpp_handle *h, const char *name, const char *value) {
    if (!h || !name || !value) return fail(PWPP_E_ARG, "null argument");
    int rc = enter(h);
    if (rc) return rc;
    const std::string k = name;
    if (k == "fit_plan") {
        for (const char *c = value; *c; ++c)
            if (!std::strchr("SWBH0123456789.:,", *c)) return fail(PWPP_E_ARG, "fit_plan '%s': unexpected character '%c'", value, *c);
        h->fit_plan = value;
    } else if (k == "one_pass") {
        h->no_one_pass = std::atoi(value) == 0;
    } else if (k == "exact_moments") {
        // the width of the plane-fit sums (include/pwpp.h): "1" = contract v4, a 2^-30 m grid; "0" = rounds 3-5's 2^-21 m grid.
        // The per-bin origins do not depend on it; shift and z half-range do.
        const int v = std::atoi(value);
        if ((v != 0 && v != 1) || (value[0] != '0' && value[0] != '1') || value[1] != 0) return fail(PWPP_E_ARG, "exact_moments=%s: 0 or 1 expected", value);
        std::vector<float2> origin;
        h->dp.fxp_wide = v;
        h->dp.fxp_zr = (float)fxp_geometry(h->dp, origin, h->dp.fxp_shift, v != 0);
    } else if (k == "split_k5") {
        const int v = std::atoi(value);
        if (v < 0 || v > 2) return fail(PWPP_E_ARG, "split_k5=%s: 0, 1 or 2 expected", value);
        h->split_k5 = v;
    } else if (k == "redo_whole_batch") {
        h->redo_whole_batch = std::atoi(value) != 0;
    } else if (k == "one_pass_min_frames") {
        const int v = std::atoi(value);
        if (v < 1) return fail(PWPP_E_ARG, "one_pass_min_frames=%s: >= 1 expected", value);
        h->one_pass_min_frames = h->one_pass_min_fresh = v;
    } else if (k == "one_pass_scale") {
        const double v = std::atof(value);
        if (!(v > 0.0 && v <= 1024.0)) return fail(PWPP_E_ARG, "one_pass_scale=%s: a positive number up to 1024 expected", value);
        h->one_pass_scale = v;
        h->table_stale = true;  // rebuild the capacity table
    } else if (k == "fit_streams") {
        const int v = std::atoi(value);
        if (v < 1 || v > 8) return fail(PWPP_E_ARG, "fit_streams=%s: 1..8 expected", value);
        h->num_fit_streams = v;
    } else if (k == "overlap_ranges") {
        const int v = std::atoi(value);
        if (v < 2 || v > 64) return fail(PWPP_E_ARG, "overlap_ranges=%s: 2..64 expected", value);
        h->overlap_ranges = v;
    } else if (k == "hi_split") {
        // height over the ground level where the high part of a bin begins (pwpp_dev.h); results never depend on it
        const double v = std::atof(value);
        if (!(v >= -1e30 && v <= 1e30)) return fail(PWPP_E_ARG, "hi_split=%s: a number of metres expected (1e30: no high parts)", value);
        h->dp.hi_split = (float)v;
        HIPCHK(hipMemsetAsync(h->d_bin_max.p, 0, (size_t)PWPP_NUM_PARTS(h->dp.num_bins) * sizeof(uint32_t), h->stream));
        h->have_observation = false;  // the parts change: size the one-pass segments anew
        h->table_stale = true;
    } else if (k == "hi_split_zones") {
        const int v = std::atoi(value);
        if (v < 0 || v > 4) return fail(PWPP_E_ARG, "hi_split_zones=%s: 0..4 expected", value);
        h->dp.split_end = h->dp.bin_base[v];
        HIPCHK(hipMemsetAsync(h->d_bin_max.p, 0, (size_t)PWPP_NUM_PARTS(h->dp.num_bins) * sizeof(uint32_t), h->stream));
        h->have_observation = false;
        h->table_stale = true;
    } else if (const PathOption *o = path_option(k)) {
        const int v = std::atoi(value);
        if (v < 0 || v > o->max) return fail(PWPP_E_ARG, o->max == 1 ? "%s=%s: 0 or 1 expected" : "%s=%s: 0, 1 or 2 expected", o->name, value);
        h->*(o->member) = v;
    } else if (k == "debug_flags") {
        const int v = std::atoi(value);
        //  the fit-chain probes (4) and the binning / scan / GLE probes (8) write the same 64-entry array
        if ((v & 4) && (v & 8)) return fail(PWPP_E_ARG, "debug_flags=%s: the timing probes 4 and 8 share one probe array; set one of them", value);
        h->debug_flags = v;
    } else {
        return fail(PWPP_E_ARG, "unknown option '%s'", name);
    }
    return PWPP_OK;
}

int64_t pwpp_get_workspace_bytes(pwpp_handle *h) {
    if (!h) return PWPP_E_ARG;
    // EVERY device allocation of the handle (the sum used to leave out the descriptors, the stream state and
    // the tables, and reported the per-frame buffers pwpp_trim_workspace did not free)
    int64_t sum = 0;
    for (const BufBase *b : h->bufs)
        if (b->on_device) sum += (int64_t)b->bytes();
    return sum;
}

int pwpp_trim_workspace(pwpp_handle *h) {
    int rc = enter(h);
    if (rc) return rc;
    // everything whose size follows the batch: inputs, bin-ordered planes, lists, per-frame tables and records, the state of
    // FRESH frames and the snapshots of a one-pass batch.  What stays: the streams' state (thresholds, histories, plane
    // members), the per-handle tables (origins, boxes, segment table, largest counts) and 512 bytes of timing probes.
    for (BufBase *b : h->bufs)
        if (b->per_batch) b->release();
    h->have_results = false;  // the index lists lived in d_out, the records in d_recs
    h->ground_rows_valid = false;
    h->next_clean.valid = false;  // (the counters' copies are gone with d_parts / d_results)
    h->descs_on_device.clear();
    return PWPP_OK;
}

int pwpp_set_output_order(pwpp_handle *h, int order) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (order != PWPP_ORDER_SCATTER && order != PWPP_ORDER_REFERENCE && order != PWPP_ORDER_CLOUD) return fail(PWPP_E_ARG, "bad order %d", order);
    int rc = enter(h);
    if (rc) return rc;
    h->output_order = order;
    return PWPP_OK;
}

int pwpp_set_labels(pwpp_handle *h, int on) { return set_output(h, kLabels, on); }
int pwpp_set_point_planes(pwpp_handle *h, int on) { return set_output(h, kPointPlanes, on); }
int pwpp_set_point_records(pwpp_handle *h, int on) { return set_output(h, kPointRecords, on); }

int pwpp_set_input_transforms(pwpp_handle *h, const float *T, int count) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (count < 0 || count > 65535) return fail(PWPP_E_ARG, "count=%d: 0 ... 65535 transforms expected", count);
    const size_t floats = T ? 12 * (size_t)count : 0;
    for (size_t k = 0; k < floats; ++k)
        if (!std::isfinite(T[k])) return fail(PWPP_E_ARG, "transform %zu, entry %zu is not finite", k / 12, k % 12);
    const int rc = enter(h);
    if (rc) return rc;
    h->input_xf.assign(T, T + floats);  // (d_xf keeps what the last call ran with until the next estimate call: its lazy gathers use that)
    return PWPP_OK;
}

int pwpp_transform_points(const float T[12], const float *xyz, int64_t m, float *out) {
    if (m < 0 || !T || (m > 0 && (!xyz || !out))) return fail(PWPP_E_ARG, "null argument or negative count");
    for (int64_t i = 0; i < m; ++i) {
        float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        pwpp_transform_point(T, x, y, z);
        out[3 * i] = x;
        out[3 * i + 1] = y;
        out[3 * i + 2] = z;
    }
    return PWPP_OK;
}

int pwpp_get_labels(pwpp_handle *h, int frame, uint8_t *out) {
    return copy_output(h, kLabels, frame, false, out, h ? h->d_labels.p : nullptr, 1);
}
int pwpp_get_all_labels(pwpp_handle *h, uint8_t *out) {
    return copy_output(h, kLabels, 0, true, out, h ? h->d_labels.p : nullptr, 1);
}
int pwpp_get_point_patches(pwpp_handle *h, int frame, int32_t *out) {
    return copy_output(h, kPointPlanes, frame, false, out, h ? h->d_pt_patch.p : nullptr, sizeof(int32_t));
}
int pwpp_get_point_distances(pwpp_handle *h, int frame, float *out) {
    return copy_output(h, kPointPlanes, frame, false, out, h ? h->d_pt_dist.p : nullptr, sizeof(float));
}
int pwpp_get_all_point_patches(pwpp_handle *h, int32_t *out) {
    return copy_output(h, kPointPlanes, 0, true, out, h ? h->d_pt_patch.p : nullptr, sizeof(int32_t));
}
int pwpp_get_all_point_distances(pwpp_handle *h, float *out) {
    return copy_output(h, kPointPlanes, 0, true, out, h ? h->d_pt_dist.p : nullptr, sizeof(float));
}

int pwpp_get_device_labels(pwpp_handle *h, const uint8_t **out) {
    if (!h || !out) return fail(PWPP_E_ARG, "null argument");
    const int rc = need_output(h, 0, kLabels);
    if (rc) return rc;
    *out = h->d_labels.p;
    return PWPP_OK;
}

int pwpp_get_device_point_planes(pwpp_handle *h, const int32_t **patches, const float **distances) {
    if (!h || (!patches && !distances)) return fail(PWPP_E_ARG, "null argument");
    const int rc = need_output(h, 0, kPointPlanes);
    if (rc) return rc;
    if (patches) *patches = h->d_pt_patch.p;
    if (distances) *distances = h->d_pt_dist.p;
    return PWPP_OK;
}

int pwpp_get_record_bytes(pwpp_handle *h) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (h->record_bytes <= 0) return fail(PWPP_E_STATE, "no frame has been processed yet");
    return h->record_bytes;
}

// The rows of one list of one frame.  A call that ran with point records left them in d_records: a copy.  Otherwise they are
// gathered now from the frame's input, like copy_xyz (after a PWPP_MEM_DEVICE call: the caller's buffer, which must still hold it).
static int copy_records(pwpp_handle *h, int frame, void *out, bool ground) {
    int rc = check_frame(h, frame);
    if (rc) return rc;
    const PwppFrameResult &r = h->h_results.p[frame];
    const int64_t first = h->h_base.p[frame] + (ground ? 0 : r.n_ground);
    const int count = ground ? r.n_ground : r.n_nonground;
    if (count <= 0) return PWPP_OK;
    if (!out) return fail(PWPP_E_ARG, "null output");
    const size_t rb = (size_t)h->record_bytes, bytes = (size_t)count * rb;
    const uint8_t *src = h->d_records.p + (size_t)first * rb;
    if (!(h->outputs_last & bit(kPointRecords))) {
        // (d_xyz is the getters' gather scratch: whole floats, and 16-byte aligned for the wide pieces)
        if ((rc = h->d_xyz.ensure((bytes + 3) / 4))) return rc;
        const int lrc = pwpp_launch_gather_records(&h->descs[(size_t)frame], h->d_out.p + first, count, h->d_xyz.p, h->records_path, h->stream);
        if (lrc != 0) return fail(PWPP_E_HIP, "gather launch failed: %s", hipGetErrorString((hipError_t)lrc));
        src = reinterpret_cast<const uint8_t *>(h->d_xyz.p);
    }
    HIPCHK(hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return PWPP_OK;
}
int pwpp_get_ground_records(pwpp_handle *h, int frame, void *out) { return copy_records(h, frame, out, true); }
int pwpp_get_nonground_records(pwpp_handle *h, int frame, void *out) { return copy_records(h, frame, out, false); }

int pwpp_get_all_records(pwpp_handle *h, void *out, int64_t *frame_base, int32_t *counts) {
    const int rc = copy_output(h, kPointRecords, 0, true, out, h ? h->d_records.p : nullptr, h ? (size_t)h->record_bytes : 0);
    if (rc) return rc;
    if (frame_base) std::memcpy(frame_base, h->h_base.p, ((size_t)h->frames + 1) * sizeof(int64_t));
    if (counts) std::memcpy(counts, h->h_results.p, (size_t)h->frames * sizeof(PwppFrameResult));
    return PWPP_OK;
}

int pwpp_get_device_records(pwpp_handle *h, const void **out, int32_t *record_bytes) {
    if (!h || (!out && !record_bytes)) return fail(PWPP_E_ARG, "null argument");
    const int rc = need_output(h, 0, kPointRecords);
    if (rc) return rc;
    if (out) *out = h->d_records.p;
    if (record_bytes) *record_bytes = h->record_bytes;
    return PWPP_OK;
}

// ---- ground queries: the last call's planes at arbitrary positions -------------------------------------------------------
namespace {
// The last call's results as the ground-query kernels see them.  The bin -> row table is allocated here, on the first query, and
// computed here: once per estimate call, before the first kernel that reads the rows.
int ground_view(pwpp_handle *h, PwppGroundView &v) {
    const int32_t *const held = h->d_ground_rows.p;
    const int rc = h->d_ground_rows.ensure((size_t)h->frames * (size_t)h->dp.num_bins);
    if (h->d_ground_rows.p != held) h->ground_rows_valid = false;
    if (rc) return rc;
    std::memset(&v, 0, sizeof(v));
    v.P = h->dp;
    v.bin_count = h->d_bins.p;  // (the first slab: fill_batch)
    v.recs = h->d_recs.p;
    v.rows = h->d_ground_rows.p;
    v.num_frames = h->frames;
    v.debug = h->debug_flags;
    if (!h->ground_rows_valid) {
        const int lrc = pwpp_launch_ground_rows(&v, h->stream);
        if (lrc != 0) return launch_failed(h, lrc);
        h->ground_rows_valid = true;
    }
    return PWPP_OK;
}

// The memory kinds of the calls that stage their arrays; `who`: the subject and its verb, "the ground queries take".
int mem_args(int mem, const char *who) {
    if (mem == PWPP_MEM_HOST || mem == PWPP_MEM_DEVICE) return PWPP_OK;
    return fail(PWPP_E_ARG, "mem %d: %s PWPP_MEM_HOST or PWPP_MEM_DEVICE", mem, who);
}

// What a call checks of the number of things it takes one for all frames or one per frame (`noun`: "origins", "poses", "start sets") ...
int per_frame_count_args(int n, int frames, const char *noun) {
    if (n < 1 || (n != 1 && n != frames)) return fail(PWPP_E_ARG, "%d %s for %d frames: 1 or one per frame expected", n, noun, frames);
    return PWPP_OK;
}

// ... and of such a list of cells, n rows of `stride` words that begin {x, y} (3: the viewshed's, with an eye), on an image of
// nx x ny cells (`noun`: "origin", "source"): the first one outside is named
int cells_inside_args(const int32_t *xy, int n, int nx, int ny, const char *noun, int stride = 2) {
    for (int i = 0; i < n; ++i)
        if (const int32_t *c = xy + stride * i; c[0] < 0 || c[0] >= nx || c[1] < 0 || c[1] >= ny)
            return fail(PWPP_E_ARG, "%s %d, cell (%d, %d), lies outside the %d x %d cells", noun, i, c[0], c[1], nx, ny);
    return PWPP_OK;
}

// What PWPP_MEM_DEVICE asks of the caller's arrays (after mem): the first of `a` that is off its alignment, mask + 1 bytes, is named.
struct Aligned {
    const void *p;
    unsigned mask;
    const char *name;
};
int alignment_args(int mem, std::initializer_list<Aligned> a) {
    if (mem != PWPP_MEM_DEVICE) return PWPP_OK;
    for (const Aligned &x : a)
        if (reinterpret_cast<uintptr_t>(x.p) & x.mask) return fail(PWPP_E_ARG, "the %s must be %d-byte aligned", x.name, (int)x.mask + 1);
    return PWPP_OK;
}
}  // namespace

int pwpp_query_ground(pwpp_handle *h, const float *xyz, const int32_t *frame, int64_t m, int mem, pwpp_ground_sample *out) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (m < 0 || m > ((int64_t)1 << 31)) return fail(PWPP_E_ARG, "%lld positions (0..2^31 supported)", (long long)m);
    if (m > 0 && (!xyz || !out)) return fail(PWPP_E_ARG, "null %s", xyz ? "output" : "positions");
    int rc = mem_args(mem, "the ground queries take");
    if (rc) return rc;
    if ((rc = check_frame(h, 0))) return rc;
    if (m == 0) return PWPP_OK;
    const size_t um = (size_t)m;
    Staging st(h, h->d_ground_stage, mem);  // the output first: 16-byte aligned for the kernel's wide stores
    const int s_out = st.add(um * 4, out, Staging::kOut), s_xyz = st.add(um * 3, xyz, Staging::kIn), s_frame = st.add(um, frame, Staging::kIn);
    if ((rc = st.begin())) return rc;
    PwppGroundView v;
    if ((rc = ground_view(h, v))) return rc;
    const int lrc = pwpp_launch_ground_query(&v, st.dev<const float>(s_xyz), st.dev<const int32_t>(s_frame), m, st.dev<void>(s_out), h->stream);
    return lrc != 0 ? launch_failed(h, lrc) : st.end();
}

}  // extern "C"

namespace {
// What every entry point that takes a grid checks of it; reads the grid alone.
int grid_geometry_args(const pwpp_ground_grid *g) {
    if (g->nx < 1 || g->ny < 1) return fail(PWPP_E_ARG, "grid of %d x %d cells", g->nx, g->ny);
    if (!(g->cell > 0.0) || !std::isfinite(g->cell) || !std::isfinite(g->x0) || !std::isfinite(g->y0))
        return fail(PWPP_E_ARG, "grid origin and cell size must be finite, the cell size positive");
    return PWPP_OK;
}

// What the entry points over the last call's results check of their grid and frame range, in this order, after the null checks
// of their own; lands the call in flight.  `cells`: nx * ny * frames.
int ground_grid_args(pwpp_handle *h, const pwpp_ground_grid *g, int frame_first, int frames, int mem, size_t &cells) {
    int rc = grid_geometry_args(g);
    if (rc) return rc;
    if ((rc = mem_args(mem, "the ground queries take"))) return rc;
    if ((rc = check_frame(h, 0))) return rc;
    if (frame_first < 0 || frames < 1 || frames > h->frames - frame_first)
        return fail(PWPP_E_ARG, "frames [%d, %d + %d) outside the last call's [0, %d)", frame_first, frame_first, frames, h->frames);
    const int64_t per_frame = (int64_t)g->nx * (int64_t)g->ny;  // (< 2^62)
    if (per_frame > ((int64_t)1 << 31) / frames) return fail(PWPP_E_ARG, "%d x %d cells x %d frames exceed 2^31", g->nx, g->ny, frames);
    cells = (size_t)per_frame * (size_t)frames;
    return PWPP_OK;
}

// ... of the grid's flags and the height band of a counted point (the three entry points over the non-ground lists) ...
int obstacle_band_args(const pwpp_ground_grid *g, float h_min, float h_max) {
    if (g->flags & ~(int32_t)PWPP_GRID_GROUND_ONLY) return fail(PWPP_E_ARG, "grid flags %d: 0 or PWPP_GRID_GROUND_ONLY", g->flags);
    if (!(h_min <= h_max)) return fail(PWPP_E_ARG, "height band [%g, %g]: h_min <= h_max expected, neither a NaN", (double)h_min, (double)h_max);
    return PWPP_OK;
}

// ... of one frame's cells where a cell index is an int32 (labels, the cluster table's first_cell) ...
int frame_cells_args(int nx, int ny) {
    if ((int64_t)nx * (int64_t)ny > (int64_t)INT32_MAX) return fail(PWPP_E_ARG, "%d x %d cells exceed 2^31 - 1", nx, ny);
    return PWPP_OK;
}

// ... of an image's sides where a coordinate has 15 bits (distances: the largest dist2, 2 * 32767^2, stays below
// PWPP_DIST_BEYOND; visibility); `who` as in mem_args ...
static_assert(PWPP_DIST_MAX_SIDE == 32768 && PWPP_VIS_MAX_SIDE == 32768, "the side limit of the message");
int side_args(int nx, int ny, const char *who) {
    if (nx > 32768 || ny > 32768) return fail(PWPP_E_ARG, "%d x %d cells: %s at most 32768 a side", nx, ny, who);
    return PWPP_OK;
}

// ... and of the occupancy threshold (every operator on an occupancy image)
int min_count_args(int min_count) {
    if (min_count < 1) return fail(PWPP_E_ARG, "min_count %d: at least 1 expected", min_count);
    return PWPP_OK;
}

// What the pwpp_*_grid entry points check of the shape of the caller's images.  `side_who`: the operator takes at most 32768 cells
// a side (side_args); null: it indexes one frame's cells with an int32 (frame_cells_args).  `cells`: nx * ny * frames.
int image_args(int nx, int ny, int frames, const char *side_who, size_t &cells) {
    if (nx < 1 || ny < 1 || frames < 1) return fail(PWPP_E_ARG, "%d frames of %d x %d cells", frames, nx, ny);
    if (const int rc = side_who ? side_args(nx, ny, side_who) : frame_cells_args(nx, ny)) return rc;
    const int64_t per_frame = (int64_t)nx * (int64_t)ny;
    if (per_frame > ((int64_t)1 << 31) / frames) return fail(PWPP_E_ARG, "%d x %d cells x %d frames exceed 2^31", nx, ny, frames);
    cells = (size_t)per_frame * (size_t)frames;
    return PWPP_OK;
}

// "The non-ground lists of frames [frame_first, frame_first + frames) of the last call over the grid g", as the kernels take it
// (PwppObstacleScan); the arguments are checked.  Everything those kernels read is on the device since the call: the frame
// descriptors (d_frames), this call's copy of the frame counters (d_results), the lists (d_out) -- and the INPUT, which after a
// PWPP_MEM_DEVICE call is the caller's buffer (the lifetime rule of pwpp_get_nonground_xyz).
int obstacle_scan(pwpp_handle *h, const pwpp_ground_grid *g, float h_min, float h_max, int frame_first, int frames, PwppObstacleScan &s) {
    std::memset(&s, 0, sizeof(s));
    const int rc = ground_view(h, s.Q);
    if (rc) return rc;
    s.descs = h->d_frames.p;
    s.results = h->d_results.p + (size_t)h->counters_copy * (size_t)h->frames;
    s.out_idx = h->d_out.p;
    std::memcpy(&s.G, g, sizeof(s.G));
    s.frame_first = frame_first, s.frames = frames;
    for (int f = frame_first; f < frame_first + frames; ++f) s.max_nonground = std::max(s.max_nonground, h->h_results.p[f].n_nonground);
    s.h_min = h_min, s.h_max = h_max;
    return PWPP_OK;
}

// ---- operators on an occupancy image: clusters, distances, visibility, fusion, scan match ----------------------------------------
// Each has two entry points: pwpp_*_grid works on the caller's image, pwpp_*_obstacles on the one it first rasterises from the last call's
// non-ground lists.  An operator states its sections once (*_sections: the kernels' working words and the tables the call built for them
// first -- upload sections, copied by Staging::begin() -- then what the call stages) and its launch once (*_launch: the launcher's call alone);
// an entry point checks its arguments, declares the sections and runs one of five tails: run_on_image, run_on_obstacles, run_on_visibility
// (further down: the obstacle tail under the visibility operator), run_on_labels (further down: the obstacle tail under the labelling and its per-point
// scatter, for the tracks and the map evidence), run_on_ground (the elevation fusion, the terrain and the reach on the ground raster).
// The costmap's chain needs both rasters in one staging: it enqueues what run_on_obstacles and run_on_ground enqueue (enqueue_on_*) between one begin() and one end().
// Stated once for all of them: a count given "1 or one per frame" (per_frame_count_args) and a list of cells inside the image (cells_inside_args), a byte
// image's section (Staging::add_bytes), the first checks of a labelling (label_first_args) and of a reach on a caller's image (reach_image_args), the
// terrain analysis as a stage for its cost bytes alone (terrain_cost_sections), the reach's sections for the field and for the routes (reach_sections).
// The two lines of sight share the checks of their chained calls (visibility_origin_args), origins with or without a height (cells_inside_args, frame_cells_of, frame_cells_section)
// and the ground returns' launch (enqueue_ground_returns); boxes and hulls, the row tables of a label image: row_table_args, row_table_obstacle_args, row_table_launches, counted_points.

// The section of an operator's input image (count, top).  From the caller (pwpp_*_grid): read, and absent without a pointer.
// From the raster (pwpp_*_obstacles): written for the caller who asks for it, else kept in the buffer.
int add_image(Staging &st, size_t cells, const void *user, bool from_raster) {
    if (from_raster) return st.add(cells, user, user ? Staging::kOut : Staging::kKept);
    return st.add(user ? cells : 0, user, Staging::kIn);
}

// On a caller's image.  Like a getter, the call in flight lands first; no results are needed.
template <class Op>
int run_on_image(pwpp_handle *h, Staging &st, Op op) {
    int rc = enter(h, true);
    if (rc || (rc = st.begin())) return rc;
    const int lrc = op();
    return lrc != 0 ? launch_failed(h, lrc) : st.end();
}

// What run_on_obstacles enqueues between st.begin() and st.end(): the raster and `op`.  On its own for a call that chains both rasters
// in one staging (the costmap).
template <class Op>
int enqueue_on_obstacles(pwpp_handle *h, Staging &st, const pwpp_ground_grid *g, float h_min, float h_max, int frame_first, int frames, int s_count, int s_top,
                         Op op) {
    PwppObstacleScan scan;
    if (const int rc = obstacle_scan(h, g, h_min, h_max, frame_first, frames, scan)) return rc;
    int lrc = pwpp_launch_obstacle_raster(&scan, st.dev<int32_t>(s_count), s_top < 0 ? nullptr : st.dev<float>(s_top), nullptr, h->stream);
    if (lrc == 0) lrc = op(scan);
    return lrc != 0 ? launch_failed(h, lrc) : PWPP_OK;
}

// On the obstacle grid: pwpp_rasterize_obstacles into the sections s_count and (-1: none) s_top, then the operator and whatever
// the entry point appends (`op`: it sees the scan and returns a HIP error code), enqueued as one sequence.
template <class Op>
int run_on_obstacles(pwpp_handle *h, Staging &st, const pwpp_ground_grid *g, float h_min, float h_max, int frame_first, int frames, int s_count, int s_top,
                     Op op) {
    int rc = st.begin();
    if (rc || (rc = enqueue_on_obstacles(h, st, g, h_min, h_max, frame_first, frames, s_count, s_top, op))) return rc;
    return st.end();
}

// What run_on_ground enqueues between st.begin() and st.end(), as enqueue_on_obstacles is to run_on_obstacles.
template <class Op>
int enqueue_on_ground(pwpp_handle *h, Staging &st, const pwpp_ground_grid *g, int frame_first, int frames, int s_height, int s_patch, Op op) {
    PwppGroundView v;
    PwppGroundGrid grid;
    std::memcpy(&grid, g, sizeof(grid));
    if (const int rc = ground_view(h, v)) return rc;
    int lrc = pwpp_launch_ground_raster(&v, &grid, frame_first, frames, st.dev<float>(s_height), s_patch < 0 ? nullptr : st.dev<int32_t>(s_patch), h->stream);
    if (lrc == 0) lrc = op();
    return lrc != 0 ? launch_failed(h, lrc) : PWPP_OK;
}

// On the ground raster: pwpp_rasterize_ground into the sections s_height and (-1: none) s_patch, then `op` (a HIP error code), one sequence.
template <class Op>
int run_on_ground(pwpp_handle *h, Staging &st, const pwpp_ground_grid *g, int frame_first, int frames, int s_height, int s_patch, Op op) {
    int rc = st.begin();
    if (rc || (rc = enqueue_on_ground(h, st, g, frame_first, frames, s_height, s_patch, op))) return rc;
    return st.end();
}

// What the operators on the ground raster check first of the frames and the grid, before their own arguments; `who` as in mem_args.
int ground_first_args(const pwpp_ground_grid *g, int frames, const char *who) {
    if (frames < 1 || g->nx < 1 || g->ny < 1) return fail(PWPP_E_ARG, "%d frames of %d x %d cells", frames, g->nx, g->ny);
    if (const int rc = side_args(g->nx, g->ny, who)) return rc;
    if (g->flags & ~(int32_t)PWPP_GRID_GROUND_ONLY) return fail(PWPP_E_ARG, "grid flags %d: 0 or PWPP_GRID_GROUND_ONLY", g->flags);
    return PWPP_OK;
}
}  // namespace

extern "C" {

int pwpp_rasterize_ground(pwpp_handle *h, const pwpp_ground_grid *g, int frame_first, int frames, int mem, float *height, int32_t *patch) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!g || !height) return fail(PWPP_E_ARG, "null %s", g ? "height image" : "grid");
    size_t cells = 0;
    int rc = ground_grid_args(h, g, frame_first, frames, mem, cells);
    if (rc) return rc;
    Staging st(h, h->d_ground_stage, mem);
    const int s_height = st.add(cells, height, Staging::kOut), s_patch = st.add(patch ? cells : 0, patch, Staging::kOut);
    return run_on_ground(h, st, g, frame_first, frames, s_height, s_patch, [] { return 0; });
}

// The non-ground points of the last call per cell of the grid: count, then top, then unref.
int pwpp_rasterize_obstacles(pwpp_handle *h, const pwpp_ground_grid *g, float h_min, float h_max, int frame_first, int frames, int mem,
                             int32_t *count, float *top, int32_t *unref) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!g || !count) return fail(PWPP_E_ARG, "null %s", g ? "count image" : "grid");
    int rc = obstacle_band_args(g, h_min, h_max);
    if (rc) return rc;
    size_t cells = 0;
    if ((rc = ground_grid_args(h, g, frame_first, frames, mem, cells))) return rc;
    Staging st(h, h->d_ground_stage, mem);
    const int s_count = st.add(cells, count, Staging::kOut), s_top = st.add(top ? cells : 0, top, Staging::kOut);
    const int s_unref = st.add(unref ? cells : 0, unref, Staging::kOut);
    if ((rc = st.begin())) return rc;
    PwppObstacleScan scan;
    if ((rc = obstacle_scan(h, g, h_min, h_max, frame_first, frames, scan))) return rc;
    const int lrc = pwpp_launch_obstacle_raster(&scan, st.dev<int32_t>(s_count), st.dev<float>(s_top), st.dev<int32_t>(s_unref), h->stream);
    return lrc != 0 ? launch_failed(h, lrc) : st.end();
}

// ---- obstacle clusters: connected occupied cells of an obstacle grid ------------------------------------------------------------
namespace {
// what both entry points check of min_count, connectivity and the table
int cluster_param_args(int mem, int min_count, int connectivity, const void *clusters, int max_clusters) {
    if (const int rc = min_count_args(min_count)) return rc;
    if (connectivity != 4 && connectivity != 8) return fail(PWPP_E_ARG, "connectivity %d: 4 or 8 expected", connectivity);
    if (max_clusters < 0) return fail(PWPP_E_ARG, "max_clusters %d", max_clusters);
    if (max_clusters > 0 && !clusters) return fail(PWPP_E_ARG, "null cluster table with max_clusters %d", max_clusters);
    return alignment_args(mem, {{clusters, 7u, "cluster table"}});
}

constexpr size_t kClusterRowWords = sizeof(pwpp_obstacle_cluster) / 4;
static_assert(sizeof(pwpp_obstacle_cluster) == 48, "pwpp_obstacle_cluster is 48 bytes");

struct ClusterSections {
    int work, count, top, label, table, n;
};
ClusterSections cluster_sections(Staging &st, int nx, int ny, int frames, size_t cells, bool from_raster, const int32_t *count, const float *top,
                                 int32_t *label, pwpp_obstacle_cluster *clusters, int32_t *n_clusters, int max_clusters) {
    ClusterSections s;
    s.work = st.add(pwpp_cluster_work_words(nx, ny, frames), nullptr, Staging::kKept);
    s.count = add_image(st, cells, count, from_raster), s.top = add_image(st, cells, top, from_raster);
    s.label = st.add(cells, label, Staging::kOut);
    s.table = st.add((size_t)frames * (size_t)max_clusters * kClusterRowWords, clusters, Staging::kOut);
    s.n = st.add((size_t)frames, n_clusters, Staging::kOut);
    return s;
}
int cluster_launch(pwpp_handle *h, const Staging &st, const ClusterSections &s, int nx, int ny, int frames, int min_count, int connectivity, int max_clusters) {
    return pwpp_launch_label_grid(nx, ny, frames, st.dev<const int32_t>(s.count), st.dev<const float>(s.top), min_count, connectivity, h->clusters_path,
                                  st.dev<int32_t>(s.label), st.dev<void>(s.table), st.dev<int32_t>(s.n), max_clusters, st.dev<uint32_t>(s.work), h->stream);
}

// The caller's arrays of a labelling of the obstacle grid: what pwpp_label_obstacles and the entry points that append to it pass on.
struct LabelArrays {
    int32_t *label, *count;
    float *top;
    pwpp_obstacle_cluster *clusters;
    int32_t *n_clusters;
    int max_clusters;
    int32_t *point_cluster;
};

// What those entry points check first, in this order, after their null pointers; lands the call in flight.  `side_who`: the operator the entry
// point appends takes at most 32768 cells a side (side_args, `who` as in mem_args); null: nothing is appended.  `cells`: nx * ny * frames.
int label_first_args(pwpp_handle *h, const pwpp_ground_grid *g, float h_min, float h_max, int min_count, int connectivity, int frame_first, int frames, int mem,
                     const LabelArrays &a, const char *side_who, size_t &cells) {
    int rc = obstacle_band_args(g, h_min, h_max);
    if (rc) return rc;
    if ((rc = cluster_param_args(mem, min_count, connectivity, a.clusters, a.max_clusters))) return rc;
    if ((rc = ground_grid_args(h, g, frame_first, frames, mem, cells))) return rc;
    if ((rc = frame_cells_args(g->nx, g->ny))) return rc;
    return side_who ? side_args(g->nx, g->ny, side_who) : PWPP_OK;
}

// The fifth tail, for the operators on the label image of the obstacle grid: raster, labelling, the per-point scatter and the operator, as one enqueued
// sequence (run_on_obstacles).  The label image stays where it lies: the caller's, or the cluster buffer's in PWPP_MEM_HOST.  `declare` adds its sections
// behind the labelling's -- it is told the label image's -- and returns its launch; the arguments are checked (label_first_args).
extern "C++" template <class Declare>  // (the entry points' extern "C" block is open around this namespace)
int run_on_labels(pwpp_handle *h, const pwpp_ground_grid *g, float h_min, float h_max, int min_count, int connectivity, int frame_first, int frames, int mem,
                  size_t cells, const LabelArrays &a, Declare declare) {
    const int64_t base_first = h->h_base.p[frame_first];
    const size_t points = a.point_cluster ? (size_t)(h->h_base.p[frame_first + frames] - base_first) : 0;
    Staging st(h, h->d_clusters, mem, kClusterAlign);
    const ClusterSections s = cluster_sections(st, g->nx, g->ny, frames, cells, true, a.count, a.top, a.label, a.clusters, a.n_clusters, a.max_clusters);
    const int s_pc = st.add(points, a.point_cluster, Staging::kOut);
    const auto launch = declare(st, s.label);
    return run_on_obstacles(h, st, g, h_min, h_max, frame_first, frames, s.count, s.top, [&](const PwppObstacleScan &scan) {
        int lrc = cluster_launch(h, st, s, g->nx, g->ny, frames, min_count, connectivity, a.max_clusters);
        if (lrc == 0 && points != 0) {
            lrc = (int)hipMemsetAsync(st.dev<int32_t>(s_pc), 0xff, points * sizeof(int32_t), h->stream);  // (-1: every point that is not a counted one)
            if (lrc == 0) lrc = pwpp_launch_point_cluster(&scan, st.dev<int32_t>(s.label), st.dev<int32_t>(s_pc), base_first, h->stream);
        }
        return lrc != 0 ? lrc : launch();
    });
}
}  // namespace

int pwpp_label_grid(pwpp_handle *h, int nx, int ny, int frames, int mem, const int32_t *count, const float *top, int min_count, int connectivity,
                    int32_t *label, pwpp_obstacle_cluster *clusters, int32_t *n_clusters, int max_clusters) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!label || !count) return fail(PWPP_E_ARG, "null %s image", count ? "label" : "count");
    size_t cells = 0;
    int rc = image_args(nx, ny, frames, nullptr, cells);
    if (rc) return rc;
    if ((rc = cluster_param_args(mem, min_count, connectivity, clusters, max_clusters))) return rc;
    if ((rc = mem_args(mem, "the obstacle clusters take"))) return rc;
    Staging st(h, h->d_clusters, mem, kClusterAlign);
    const ClusterSections s = cluster_sections(st, nx, ny, frames, cells, false, count, top, label, clusters, n_clusters, max_clusters);
    return run_on_image(h, st, [&] { return cluster_launch(h, st, s, nx, ny, frames, min_count, connectivity, max_clusters); });
}

// (then the per-point scatter)
int pwpp_label_obstacles(pwpp_handle *h, const pwpp_ground_grid *g, float h_min, float h_max, int min_count, int connectivity, int frame_first, int frames,
                         int mem, int32_t *label, int32_t *count, float *top, pwpp_obstacle_cluster *clusters, int32_t *n_clusters, int max_clusters,
                         int32_t *point_cluster) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!g || !label) return fail(PWPP_E_ARG, "null %s", g ? "label image" : "grid");
    const LabelArrays a{label, count, top, clusters, n_clusters, max_clusters, point_cluster};
    size_t cells = 0;
    if (const int rc = label_first_args(h, g, h_min, h_max, min_count, connectivity, frame_first, frames, mem, a, nullptr, cells)) return rc;
    return run_on_labels(h, g, h_min, h_max, min_count, connectivity, frame_first, frames, mem, cells, a, [](Staging &, int) { return [] { return 0; }; });
}

// ---- obstacle distances: every cell's distance to the nearest occupied cell, and that cell ----------------------------------------
namespace {
static_assert(PWPP_DIST_BEYOND == PWPP_DIST_NONE, "PWPP_DIST_BEYOND is the kernels' PWPP_DIST_NONE");
constexpr const char *kDistanceWho = "the obstacle distances take";
// what both entry points check of min_count and max_dist
int distance_param_args(int min_count, int max_dist) {
    if (const int rc = min_count_args(min_count)) return rc;
    if (max_dist < 0 || max_dist > PWPP_DIST_MAX_CAP) return fail(PWPP_E_ARG, "max_dist %d: 0 (unlimited) .. 46340 cells expected", max_dist);
    return PWPP_OK;
}

struct DistanceSections {
    int work, count, dist2, nearest, metres;
};
DistanceSections distance_sections(Staging &st, int nx, int ny, int frames, size_t cells, bool from_raster, const int32_t *count, int32_t *dist2,
                                   int32_t *nearest, float *metres) {
    DistanceSections s;
    s.work = st.add(pwpp_distance_work_words(nx, ny, frames), nullptr, Staging::kKept);
    s.count = add_image(st, cells, count, from_raster), s.dist2 = st.add(cells, dist2, Staging::kOut);
    s.nearest = st.add(nearest ? cells : 0, nearest, Staging::kOut), s.metres = st.add(metres ? cells : 0, metres, Staging::kOut);
    return s;
}
int distance_launch(pwpp_handle *h, const Staging &st, const DistanceSections &s, int nx, int ny, int frames, int min_count, int max_dist, double cell) {
    return pwpp_launch_distance_grid(nx, ny, frames, st.dev<const int32_t>(s.count), min_count, max_dist, cell, h->distance_path, st.dev<int32_t>(s.dist2),
                                     st.dev<int32_t>(s.nearest), st.dev<float>(s.metres), st.dev<uint32_t>(s.work), h->stream);
}
}  // namespace

int pwpp_distance_grid(pwpp_handle *h, int nx, int ny, int frames, int mem, const int32_t *count, int min_count, int max_dist, double cell, int32_t *dist2,
                       int32_t *nearest, float *metres) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!count || !dist2) return fail(PWPP_E_ARG, "null %s image", count ? "dist2" : "count");
    size_t cells = 0;
    int rc = image_args(nx, ny, frames, kDistanceWho, cells);
    if (rc) return rc;
    if ((rc = distance_param_args(min_count, max_dist))) return rc;
    if (metres && (!(cell > 0.0) || !std::isfinite(cell))) return fail(PWPP_E_ARG, "cell size %g: finite and positive expected with a metres image", cell);
    if ((rc = mem_args(mem, kDistanceWho))) return rc;
    Staging st(h, h->d_clusters, mem, kClusterAlign);
    const DistanceSections s = distance_sections(st, nx, ny, frames, cells, false, count, dist2, nearest, metres);
    return run_on_image(h, st, [&] { return distance_launch(h, st, s, nx, ny, frames, min_count, max_dist, cell); });
}

int pwpp_distance_obstacles(pwpp_handle *h, const pwpp_ground_grid *g, float h_min, float h_max, int min_count, int max_dist, int frame_first, int frames,
                            int mem, int32_t *dist2, int32_t *nearest, float *metres, int32_t *count) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!g || !dist2) return fail(PWPP_E_ARG, "null %s", g ? "dist2 image" : "grid");
    int rc = obstacle_band_args(g, h_min, h_max);
    if (rc) return rc;
    if ((rc = side_args(g->nx, g->ny, kDistanceWho))) return rc;
    if ((rc = distance_param_args(min_count, max_dist))) return rc;
    size_t cells = 0;
    if ((rc = ground_grid_args(h, g, frame_first, frames, mem, cells))) return rc;  // (the cell size of metres is the grid's: finite and positive)
    Staging st(h, h->d_clusters, mem, kClusterAlign);
    const DistanceSections s = distance_sections(st, g->nx, g->ny, frames, cells, true, count, dist2, nearest, metres);
    return run_on_obstacles(h, st, g, h_min, h_max, frame_first, frames, s.count, -1, [&](const PwppObstacleScan &) {
        return distance_launch(h, st, s, g->nx, g->ny, frames, min_count, max_dist, g->cell);
    });
}

// ---- line-of-sight free space: the first occupied cell between the sensor's cell and every cell, and the tri-state byte ----------
namespace {
static_assert(PWPP_VIS_NONE == PWPP_VIS_FIRST_NONE && PWPP_VIS_BEYOND == PWPP_VIS_FIRST_BEYOND, "the kernels' values of first");
static_assert(PWPP_OCC_FREE == PWPP_VIS_FREE && PWPP_OCC_OCCUPIED == PWPP_VIS_OCCUPIED && PWPP_OCC_UNKNOWN == PWPP_VIS_UNKNOWN, "the kernels' occupancy bytes");
constexpr const char *kVisibilityWho = "the visibility takes";
// what both entry points check of min_count and max_range
int visibility_param_args(int min_count, int max_range) {
    if (const int rc = min_count_args(min_count)) return rc;
    if (max_range < 0 || max_range > PWPP_VIS_MAX_SIDE) return fail(PWPP_E_ARG, "max_range %d: 0 (unlimited) .. 32768 cells expected", max_range);
    return PWPP_OK;
}

// Positions in metres, one per frame or one for all (the visibility's origins, the reach's sources; `what` names one), as cells of
// the checked grid by the raster's cell rule: `out`: n x {ix, iy}.  `cols` 3 (the viewshed's origins): n x {x, y, z}, z finite too -> {ix, iy, pwpp_view_units(z)}.
int frame_cells_of(const pwpp_ground_grid *g, const double *xy, int n, const char *what, std::vector<int32_t> &out, int cols = 2) {
    out.assign((size_t)cols * (size_t)n, 0);
    for (int i = 0; i < n; ++i) {
        const double x = xy[cols * i], y = xy[cols * i + 1], z = cols == 3 ? xy[cols * i + 2] : 0.0;
        int ox = 0, oy = 0;
        if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z))
            return cols == 3 ? fail(PWPP_E_ARG, "%s %d, (%g, %g, %g), is not finite", what, i, x, y, z) : fail(PWPP_E_ARG, "%s %d, (%g, %g), is not finite", what, i, x, y);
        if (!pwpp_vis_cell_of(x, g->x0, g->cell, g->nx, ox) || !pwpp_vis_cell_of(y, g->y0, g->cell, g->ny, oy))
            return fail(PWPP_E_ARG, "%s %d, (%g, %g) m, lies outside the grid", what, i, x, y);
        out[cols * i] = ox, out[cols * i + 1] = oy;
        if (cols == 3) out[cols * i + 2] = pwpp_view_units(z);
    }
    return PWPP_OK;
}

// What the entry points that rasterise first check of the band, the grid, min_count, max_range and the origins in metres, which they turn into cells (`org`:
// n_origins x {ox, oy}).  With `min_seen` the call is the viewshed's (`who`): min_seen is checked in its place, the origins carry a height ({ox, oy, eye}).
int visibility_origin_args(const pwpp_ground_grid *g, float h_min, float h_max, int min_count, const double *origin, int n_origins, int max_range, int frames,
                           std::vector<int32_t> &org, const char *who = kVisibilityWho, const int *min_seen = nullptr) {
    int rc = obstacle_band_args(g, h_min, h_max);
    if (rc || (rc = grid_geometry_args(g))) return rc;  // (the origins need the grid)
    if ((rc = side_args(g->nx, g->ny, who))) return rc;
    if ((rc = visibility_param_args(min_count, max_range))) return rc;
    if (min_seen && *min_seen < 0) return fail(PWPP_E_ARG, "min_seen %d: 0 (no ground returns) or more expected", *min_seen);
    if ((rc = per_frame_count_args(n_origins, frames, "origins"))) return rc;
    return frame_cells_of(g, origin, n_origins, "origin", org, min_seen ? 3 : 2);
}

// The section of the cells given one per frame (the visibility's and the viewshed's origins, the reach's sources): n rows of
// `cols` words as an upload; one row travels as arguments of the launch and has no words.
int frame_cells_section(Staging &st, const std::vector<int32_t> &xy, size_t cols = 2) {
    return xy.size() > cols ? st.add_upload(std::vector<uint32_t>(xy.begin(), xy.end())) : st.add(0, nullptr, Staging::kKept);
}

// (the kernels' bit image and the origins first; `org`: the origin cells, n_origins x {ox, oy}, checked; `keep`: an image the
// caller gives no pointer for still lies in the buffer -- the fusion reads it there)
struct VisibilitySections {
    int work, org, count, first, occ;
};
VisibilitySections visibility_sections(pwpp_handle *h, Staging &st, int nx, int ny, int frames, size_t cells, bool from_raster, const int32_t *count,
                                       const std::vector<int32_t> &org, int32_t *first, int8_t *occupancy, bool keep = false) {
    VisibilitySections s;
    s.work = st.add(pwpp_visibility_work_words(nx, ny, frames, h->visibility_path), nullptr, Staging::kKept);
    s.org = frame_cells_section(st, org);
    s.count = add_image(st, cells, count, from_raster), s.first = st.add(cells, first, keep && !first ? Staging::kKept : Staging::kOut);
    s.occ = st.add_bytes(cells, occupancy, keep && !occupancy ? Staging::kKept : Staging::kOut);
    return s;
}
// (one origin travels as an argument; one per frame lies in its section)
int visibility_launch(pwpp_handle *h, const Staging &st, const VisibilitySections &s, int nx, int ny, int frames, int min_count,
                      const std::vector<int32_t> &org, int max_range) {
    return pwpp_launch_visibility_grid(nx, ny, frames, st.dev<const int32_t>(s.count), min_count, org[0], org[1], org.size() > 2 ? st.dev<const int32_t>(s.org) : nullptr,
                                       max_range, h->visibility_path, st.dev<int32_t>(s.first), st.dev<int8_t>(s.occ), st.dev<uint32_t>(s.work), h->stream);
}

// ... and an entry point that looks before its own operator: then frames >= 1 (the operator's checks come before the handle's, which would name the frames)
int visibility_first_args(const pwpp_ground_grid *g, float h_min, float h_max, int min_count, const double *origin_xy, int n_origins, int max_range, int frames,
                          std::vector<int32_t> &org) {
    const int rc = visibility_origin_args(g, h_min, h_max, min_count, origin_xy, n_origins, max_range, frames, org);
    return rc || frames >= 1 ? rc : fail(PWPP_E_ARG, "%d frames", frames);
}

// The third tail, for the operators on the visibility's bytes of the obstacle grid: raster, visibility -- count and first kept in the cluster buffer, the
// bytes too unless the caller asks for them -- and the operator, as one enqueued sequence.  `declare` adds its sections behind the visibility's and returns its launch.
extern "C++" template <class Declare>  // (the entry points' extern "C" block is open around this namespace)
int run_on_visibility(pwpp_handle *h, const pwpp_ground_grid *g, float h_min, float h_max, int min_count, const std::vector<int32_t> &org, int max_range,
                      int frame_first, int frames, int mem, size_t cells, int8_t *occupancy, Declare declare) {
    Staging st(h, h->d_clusters, mem, kClusterAlign);
    const VisibilitySections v = visibility_sections(h, st, g->nx, g->ny, frames, cells, true, nullptr, org, nullptr, occupancy, true);
    const auto launch = declare(st, v.occ);
    return run_on_obstacles(h, st, g, h_min, h_max, frame_first, frames, v.count, -1, [&](const PwppObstacleScan &) {
        const int lrc = visibility_launch(h, st, v, g->nx, g->ny, frames, min_count, org, max_range);
        return lrc != 0 ? lrc : launch();
    });
}
}  // namespace

int pwpp_visibility_grid(pwpp_handle *h, int nx, int ny, int frames, int mem, const int32_t *count, int min_count, const int32_t *origin, int n_origins,
                         int max_range, int32_t *first, int8_t *occupancy) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!count || !first || !origin) return fail(PWPP_E_ARG, "null %s", !count ? "count image" : (!first ? "first image" : "origin"));
    size_t cells = 0;
    int rc = image_args(nx, ny, frames, kVisibilityWho, cells);
    if (rc) return rc;
    if ((rc = visibility_param_args(min_count, max_range))) return rc;
    if ((rc = per_frame_count_args(n_origins, frames, "origins"))) return rc;
    if ((rc = cells_inside_args(origin, n_origins, nx, ny, "origin"))) return rc;
    if ((rc = mem_args(mem, kVisibilityWho))) return rc;
    const std::vector<int32_t> org(origin, origin + 2 * (size_t)n_origins);
    Staging st(h, h->d_clusters, mem, kClusterAlign);
    const VisibilitySections s = visibility_sections(h, st, nx, ny, frames, cells, false, count, org, first, occupancy);
    return run_on_image(h, st, [&] { return visibility_launch(h, st, s, nx, ny, frames, min_count, org, max_range); });
}

int pwpp_visibility_obstacles(pwpp_handle *h, const pwpp_ground_grid *g, float h_min, float h_max, int min_count, const double *origin_xy, int n_origins,
                              int max_range, int frame_first, int frames, int mem, int32_t *first, int8_t *occupancy, int32_t *count) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!g || !first || !origin_xy) return fail(PWPP_E_ARG, "null %s", !g ? "grid" : (!first ? "first image" : "origin"));
    std::vector<int32_t> org;
    size_t cells = 0;
    int rc = visibility_origin_args(g, h_min, h_max, min_count, origin_xy, n_origins, max_range, frames, org);
    if (rc || (rc = ground_grid_args(h, g, frame_first, frames, mem, cells))) return rc;
    Staging st(h, h->d_clusters, mem, kClusterAlign);
    const VisibilitySections s = visibility_sections(h, st, g->nx, g->ny, frames, cells, true, count, org, first, occupancy);
    return run_on_obstacles(h, st, g, h_min, h_max, frame_first, frames, s.count, -1, [&](const PwppObstacleScan &) {
        return visibility_launch(h, st, s, g->nx, g->ny, frames, min_count, org, max_range);
    });
}

// ---- viewshed: the visibility's walk with heights -- the nearest cell that hides, the lowest height seen, the tri-state byte ---------
namespace {
static_assert(PWPP_VIEW_NO_HEIGHT == PWPP_VIEW_NONE_HEIGHT && PWPP_VIEW_MAX_RISE == PWPP_VIEW_RISE_MAX && PWPP_VIEW_UNITS_PER_M == PWPP_VIEW_UNITS,
              "the kernels' heights");
constexpr const char *kViewshedWho = "the viewshed takes";

// (the kernels' bit image and the origins first; `org`: n_origins x {ox, oy, eye}, checked.  One origin travels as arguments.)
struct ViewshedSections {
    int work, org, count, block, target, seen, first, shadow, occ;
};
void viewshed_out_sections(pwpp_handle *h, Staging &st, int nx, int ny, int frames, int max_range, const std::vector<int32_t> &org, ViewshedSections &s) {
    s.work = st.add(pwpp_viewshed_work_words(nx, ny, frames, h->viewshed_path, max_range), nullptr, Staging::kKept);
    s.org = frame_cells_section(st, org, 3);
}
int viewshed_launch(pwpp_handle *h, const Staging &st, const ViewshedSections &s, int nx, int ny, int frames, int min_count, int min_seen,
                    const std::vector<int32_t> &org, int max_range) {
    return pwpp_launch_viewshed_grid(nx, ny, frames, st.dev<const int32_t>(s.count), min_count, st.dev<const int32_t>(s.block), st.dev<const int32_t>(s.target),
                                     st.dev<const int32_t>(s.seen), min_seen, org[0], org[1], org[2], org.size() > 3 ? st.dev<const int32_t>(s.org) : nullptr,
                                     max_range, h->viewshed_path, st.dev<int32_t>(s.first), st.dev<int32_t>(s.shadow), st.dev<int8_t>(s.occ),
                                     st.dev<uint32_t>(s.work), h->stream);
}
// The longest ground list of a frame range of the last call, and the ground returns of a scan's frames into `seen` (a HIP error code)
int longest_ground_list(const pwpp_handle *h, int frame_first, int frames) {
    int max_ground = 0;
    for (int f = frame_first; f < frame_first + frames; ++f) max_ground = std::max(max_ground, h->h_results.p[f].n_ground);
    return max_ground;
}
int enqueue_ground_returns(pwpp_handle *h, const PwppObstacleScan &scan, int32_t *seen) {
    return pwpp_launch_ground_returns(&scan, longest_ground_list(h, scan.frame_first, scan.frames), seen, h->stream);
}
}  // namespace

int32_t pwpp_viewshed_units(double metres) { return pwpp_view_units(metres); }

int pwpp_viewshed_grid(pwpp_handle *h, int nx, int ny, int frames, int mem, const int32_t *count, int min_count, const int32_t *block, const int32_t *target,
                       const int32_t *seen, int min_seen, const int32_t *origin, int n_origins, int max_range, int32_t *first, int32_t *shadow,
                       int8_t *occupancy) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!count || !first || !origin) return fail(PWPP_E_ARG, "null %s", !count ? "count image" : (!first ? "first image" : "origin"));
    size_t cells = 0;
    int rc = image_args(nx, ny, frames, kViewshedWho, cells);
    if (rc) return rc;
    if ((rc = visibility_param_args(min_count, max_range))) return rc;
    if (seen && min_seen < 1) return fail(PWPP_E_ARG, "min_seen %d with a seen image: at least 1 expected", min_seen);
    if ((rc = per_frame_count_args(n_origins, frames, "origins"))) return rc;
    if ((rc = cells_inside_args(origin, n_origins, nx, ny, "origin", 3))) return rc;
    for (int i = 0; i < n_origins; ++i)
        if (origin[3 * i + 2] == PWPP_VIEW_NO_HEIGHT) return fail(PWPP_E_ARG, "origin %d: its eye is PWPP_VIEW_NO_HEIGHT", i);
    if ((rc = mem_args(mem, kViewshedWho))) return rc;
    const std::vector<int32_t> org(origin, origin + 3 * (size_t)n_origins);
    Staging st(h, h->d_clusters, mem, kClusterAlign);
    ViewshedSections s;
    viewshed_out_sections(h, st, nx, ny, frames, max_range, org, s);
    s.count = add_image(st, cells, count, false), s.block = add_image(st, cells, block, false), s.target = add_image(st, cells, target, false);
    s.seen = add_image(st, cells, seen, false);
    s.first = st.add(cells, first, Staging::kOut), s.shadow = st.add(shadow ? cells : 0, shadow, Staging::kOut);
    s.occ = st.add_bytes(cells, occupancy, Staging::kOut);
    return run_on_image(h, st, [&] { return viewshed_launch(h, st, s, nx, ny, frames, min_count, min_seen, org, max_range); });
}

// The ground list of the last call per cell of the grid.
int pwpp_rasterize_ground_returns(pwpp_handle *h, const pwpp_ground_grid *g, int frame_first, int frames, int mem, int32_t *seen) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!g || !seen) return fail(PWPP_E_ARG, "null %s", g ? "seen image" : "grid");
    if (g->flags != 0) return fail(PWPP_E_ARG, "grid flags %d: 0 expected by the ground returns", g->flags);
    size_t cells = 0;
    int rc = ground_grid_args(h, g, frame_first, frames, mem, cells);
    if (rc) return rc;
    Staging st(h, h->d_ground_stage, mem);
    const int s_seen = st.add(cells, seen, Staging::kOut);
    if ((rc = st.begin())) return rc;
    PwppObstacleScan scan;
    if ((rc = obstacle_scan(h, g, 0.0f, 0.0f, frame_first, frames, scan))) return rc;
    const int lrc = enqueue_ground_returns(h, scan, st.dev<int32_t>(s_seen));
    return lrc != 0 ? launch_failed(h, lrc) : st.end();
}

// Both rasters, the quantiser, the ground returns and the viewshed, one enqueued sequence.
int pwpp_viewshed_obstacles(pwpp_handle *h, const pwpp_ground_grid *g, float h_min, float h_max, int min_count, int min_seen, const double *origin_xyz,
                            int n_origins, int max_range, int frame_first, int frames, int mem, int32_t *first, int32_t *shadow, int8_t *occupancy,
                            int32_t *count) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!g || !first || !origin_xyz) return fail(PWPP_E_ARG, "null %s", !g ? "grid" : (!first ? "first image" : "origin"));
    std::vector<int32_t> org;
    size_t cells = 0;
    int rc = visibility_origin_args(g, h_min, h_max, min_count, origin_xyz, n_origins, max_range, frames, org, kViewshedWho, &min_seen);
    if (rc || (rc = ground_grid_args(h, g, frame_first, frames, mem, cells))) return rc;
    const int nx = g->nx, ny = g->ny;
    Staging st(h, h->d_clusters, mem, kClusterAlign);
    ViewshedSections s;
    viewshed_out_sections(h, st, nx, ny, frames, max_range, org, s);
    s.count = add_image(st, cells, count, true);
    const int s_top = st.add(cells, nullptr, Staging::kKept), s_ground = st.add(cells, nullptr, Staging::kKept);
    s.block = st.add(cells, nullptr, Staging::kKept), s.target = st.add(cells, nullptr, Staging::kKept);
    s.seen = min_seen > 0 ? st.add(cells, nullptr, Staging::kKept) : st.add(0, nullptr, Staging::kIn);  // (an absent array: a null device pointer)
    s.first = st.add(cells, first, Staging::kOut), s.shadow = st.add(shadow ? cells : 0, shadow, Staging::kOut);
    s.occ = st.add_bytes(cells, occupancy, Staging::kOut);
    if ((rc = st.begin())) return rc;
    rc = enqueue_on_obstacles(h, st, g, h_min, h_max, frame_first, frames, s.count, s_top, [&](const PwppObstacleScan &scan) {
        return min_seen > 0 ? enqueue_ground_returns(h, scan, st.dev<int32_t>(s.seen)) : 0;
    });
    if (rc) return rc;
    rc = enqueue_on_ground(h, st, g, frame_first, frames, s_ground, -1, [&] {
        const int lrc = pwpp_launch_viewshed_quantise(cells, st.dev<const float>(s_ground), st.dev<const float>(s_top), st.dev<int32_t>(s.target),
                                                      st.dev<int32_t>(s.block), h->stream);
        return lrc != 0 ? lrc : viewshed_launch(h, st, s, nx, ny, frames, min_count, min_seen, org, max_range);
    });
    return rc ? rc : st.end();
}

// ---- occupancy fusion: per-frame occupancy bytes, under a pose per frame, into persistent int16 log-odds maps --------------------
namespace {
static_assert(PWPP_OCC_FREE == PWPP_FUSE_FREE && PWPP_OCC_OCCUPIED == PWPP_FUSE_OCCUPIED && PWPP_OCC_UNKNOWN == PWPP_FUSE_UNKNOWN, "the kernel's occupancy bytes");
static_assert(sizeof(pwpp_fusion_map) == 56, "pwpp_fusion_map is 56 bytes");
constexpr const char *kFusionWho = "the fusion takes";

// What the operators on a fused map check of the map description's grid and the two cell sizes; `who` as in mem_args, `map_cells`: NX * NY * n_maps.
// (pwpp_fusion_map and pwpp_height_map begin with the same grid: `M` is either)
extern "C++" template <class M>  // (the entry points' extern "C" block is open around this namespace)
int map_grid_args(const pwpp_ground_grid *g, const M *m, int n_maps, const char *who, size_t &map_cells) {
    if (const int rc = image_args(m->nx, m->ny, n_maps, who, map_cells)) return rc;
    if (!(g->cell > 0.0) || !std::isfinite(g->cell) || !(m->cell > 0.0) || !std::isfinite(m->cell))
        return fail(PWPP_E_ARG, "cell sizes %g (frames) and %g (map): finite and positive expected", g->cell, m->cell);
    return PWPP_OK;
}

// ... and of the frames' maps (args); checked, the rule answers for frame i
struct FrameMaps {
    const int32_t *map_of_frame;  // (null: one map for all, or frame i's is map i)
    int n_maps;
    int32_t operator()(int i) const { return pwpp_map_of_frame(map_of_frame, n_maps, i); }
    int args(int frames) const {
        if (!map_of_frame && n_maps != 1 && n_maps != frames)
            return fail(PWPP_E_ARG, "null map_of_frame with %d maps for %d frames: 1 map or one per frame expected", n_maps, frames);
        for (int i = 0; map_of_frame && i < frames; ++i)
            if (map_of_frame[i] < -1 || map_of_frame[i] >= n_maps)
                return fail(PWPP_E_ARG, "map_of_frame %d names map %d: -1 (skipped) .. %d expected", i, map_of_frame[i], n_maps - 1);
        return PWPP_OK;
    }
};

// whether two of the caller's byte ranges meet (a null one meets nothing)
bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return a && b && pa < pb + nb && pb < pa + na;
}

// What an operator checks of the caller's arrays among each other: no two may meet, except that the two of a pair of `in_place`
// ({input, output} as indices, input first) may be the same array -- the update in place -- unless a shift moves a map (`moved`).
struct Range {
    const void *p;
    size_t bytes;
    const char *name;
};
int range_args(std::initializer_list<Range> ranges, std::initializer_list<std::pair<int, int>> in_place, bool moved) {
    const Range *r = ranges.begin();
    for (int i = 0, n = (int)ranges.size(); i < n; ++i)
        for (int j = i + 1; j < n; ++j) {
            if (!ranges_overlap(r[i].p, r[i].bytes, r[j].p, r[j].bytes)) continue;
            const bool pair = std::find(in_place.begin(), in_place.end(), std::make_pair(i, j)) != in_place.end();
            if (pair && r[i].p == r[j].p) {
                if (moved) return fail(PWPP_E_ARG, "%s == %s with a shift that is not {0, 0}: a shifted update needs a second array", r[j].name, r[i].name);
                continue;
            }
            return fail(PWPP_E_ARG, "%s and %s overlap%s", r[i].name, r[j].name, pair ? " without being equal" : "");
        }
    return PWPP_OK;
}

// "Frames into maps under poses" (both fusions): what a checked call hands to the kernel besides its images and own parameters -- geometry,
// counts and the words to upload: the poses, `per_pose` more doubles for each (z_offset: 1), begin[n_maps + 1], frame list, shifts (none: no words).
struct MapPlan {
    PwppFusionGeometry G;
    int n_poses = 0, n_maps = 0, listed = 0, per_pose = 0;
    bool shifted = false;  // a shift array was given ...
    bool moved = false;    // ... and moves a map: one entry is not 0
    size_t map_cells = 0;  // NX * NY * n_maps
    std::vector<uint32_t> words;
    size_t at_per_pose() const { return (size_t)n_poses * 12; }
    size_t at_begin() const { return at_per_pose() + (size_t)n_poses * 2 * (size_t)per_pose; }
    size_t at_list() const { return at_begin() + (size_t)n_maps + 1; }
    size_t at_shift() const { return at_list() + (size_t)listed; }
};

// Filled in two steps around an operator's own checks, as the documented order of rejection has it: map_grid_args, its parameters, THEN
// map_plan_args; its arrays (range_args with plan.moved), THEN map_plan_words (`extra`: n_poses * per_pose doubles, or null: zeros).
extern "C++" template <class M>  // (pwpp_fusion_map or pwpp_height_map, as in map_grid_args)
int map_plan_args(const pwpp_ground_grid *g, const M *m, int frames, int n_poses, int per_pose, const int32_t *map_of_frame, int n_maps, const int32_t *shift,
                  MapPlan &plan) {
    if (const int rc = per_frame_count_args(n_poses, frames, "poses")) return rc;
    if (const int rc = FrameMaps{map_of_frame, n_maps}.args(frames)) return rc;
    for (int k = 0; shift && k < n_maps; ++k) plan.moved = plan.moved || shift[2 * (size_t)k] != 0 || shift[2 * (size_t)k + 1] != 0;
    plan.G = PwppFusionGeometry{m->x0, m->y0, m->cell, g->x0, g->y0, g->cell, m->nx, m->ny, g->nx, g->ny, 0.0};
    pwpp_fuse_reciprocal(g->cell, plan.G.inv_cell);
    plan.n_poses = n_poses, plan.n_maps = n_maps, plan.per_pose = per_pose, plan.shifted = shift != nullptr;
    return PWPP_OK;
}
int map_plan_words(int frames, const double *pose, const double *extra, const int32_t *map_of_frame, const int32_t *shift, MapPlan &plan) {
    try {
        std::vector<int32_t> begin, list;
        pwpp_map_lists(map_of_frame, plan.n_maps, frames, begin, list);
        plan.listed = (int)list.size();
        plan.words.assign(plan.at_shift() + (shift ? 2 * (size_t)plan.n_maps : 0), 0u);
        std::memcpy(plan.words.data(), pose, (size_t)plan.n_poses * 6 * sizeof(double));
        if (extra) std::memcpy(plan.words.data() + plan.at_per_pose(), extra, (size_t)plan.n_poses * (size_t)plan.per_pose * sizeof(double));
        std::memcpy(plan.words.data() + plan.at_begin(), begin.data(), begin.size() * sizeof(int32_t));
        if (plan.listed) std::memcpy(plan.words.data() + plan.at_list(), list.data(), list.size() * sizeof(int32_t));
        if (shift) std::memcpy(plan.words.data() + plan.at_shift(), shift, 2 * (size_t)plan.n_maps * sizeof(int32_t));
    } catch (const std::bad_alloc &) {
        return fail(PWPP_E_NOMEM, "no host memory for the lists of %d maps and %d frames", plan.n_maps, frames);
    }
    return PWPP_OK;
}

// What both entry points check of the map, the poses, the frame lists, the shifts and the overlaps, in the header's order, after
// the frame images' own checks (frames >= 1); fills the plan and the parameters.  Touches no handle.
int fusion_args(const pwpp_ground_grid *g, int frames, const double *pose, int n_poses, const int32_t *map_of_frame, const pwpp_fusion_map *m, int n_maps,
                const int32_t *shift, const int16_t *map_in, const int16_t *map_out, const int8_t *map_occupancy, MapPlan &plan, PwppFusionParams &P) {
    if (const int rc = map_grid_args(g, m, n_maps, kFusionWho, plan.map_cells)) return rc;
    if (m->hit < 0 || m->hit > 32767 || m->miss < 0 || m->miss > 32767) return fail(PWPP_E_ARG, "hit %d, miss %d: 0 .. 32767 expected", m->hit, m->miss);
    if (m->l_min < -32768 || m->l_min > 0 || m->l_max < 0 || m->l_max > 32767)
        return fail(PWPP_E_ARG, "clamps l_min %d, l_max %d: -32768 <= l_min <= 0 <= l_max <= 32767 expected", m->l_min, m->l_max);
    if (m->free_at < -32768 || m->free_at >= m->occupied_at || m->occupied_at > 32767)
        return fail(PWPP_E_ARG, "thresholds free_at %d, occupied_at %d: -32768 <= free_at < occupied_at <= 32767 expected", m->free_at, m->occupied_at);
    if (const int rc = map_plan_args(g, m, frames, n_poses, 0, map_of_frame, n_maps, shift, plan)) return rc;
    const size_t map_bytes = plan.map_cells * sizeof(int16_t);
    if (const int rc = range_args({{map_in, map_bytes, "map_in"}, {map_out, map_bytes, "map_out"}}, {{0, 1}}, plan.moved)) return rc;
    if (ranges_overlap(map_occupancy, plan.map_cells, map_out, map_bytes) || ranges_overlap(map_occupancy, plan.map_cells, map_in, map_bytes))
        return fail(PWPP_E_ARG, "map_occupancy overlaps %s", ranges_overlap(map_occupancy, plan.map_cells, map_out, map_bytes) ? "map_out" : "map_in");
    P = PwppFusionParams{m->hit, m->miss, m->l_min, m->l_max, m->occupied_at, m->free_at};
    return map_plan_words(frames, pose, nullptr, map_of_frame, shift, plan);
}

// (the plan's words first: they move into the staging; `occ` is the frame bytes' section: the caller's, or the visibility's)
struct FusionSections {
    int up, occ, map_in, map_out, map_occ;
};
FusionSections fusion_sections(Staging &st, MapPlan &plan, int s_occ, const int16_t *map_in, int16_t *map_out, int8_t *map_occupancy) {
    FusionSections s;
    const size_t map_words = (plan.map_cells + 1) / 2, map_bytes = plan.map_cells * sizeof(int16_t);
    s.up = st.add_upload(std::move(plan.words));
    s.occ = s_occ;
    s.map_in = st.add(map_in ? map_words : 0, map_in, Staging::kIn, map_in ? map_bytes : 0);
    s.map_out = st.add(map_words, map_out, Staging::kOut, map_bytes);
    s.map_occ = st.add_bytes(plan.map_cells, map_occupancy, Staging::kOut);
    return s;
}
int fusion_launch(pwpp_handle *h, const Staging &st, const FusionSections &s, const MapPlan &plan, const PwppFusionParams &P, int frames) {
    const int32_t *words = st.dev<const int32_t>(s.up);
    return pwpp_launch_fuse_grid(&plan.G, &P, frames, st.dev<const int8_t>(s.occ), st.dev<const double>(s.up), plan.n_poses, plan.n_maps,
                                 words + plan.at_begin(), words + plan.at_list(), plan.listed, plan.shifted ? words + plan.at_shift() : nullptr,
                                 st.dev<const int16_t>(s.map_in), st.dev<int16_t>(s.map_out), st.dev<int8_t>(s.map_occ), h->fusion_path, h->stream);
}
}  // namespace

int pwpp_fuse_grid(pwpp_handle *h, const pwpp_ground_grid *g, int frames, int mem, const int8_t *occupancy, const double *pose, int n_poses,
                   const int32_t *map_of_frame, const pwpp_fusion_map *m, int n_maps, const int32_t *shift, const int16_t *map_in, int16_t *map_out,
                   int8_t *map_occupancy) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!g || !occupancy || !pose || !m || !map_out)
        return fail(PWPP_E_ARG, "null %s", !g ? "grid" : (!occupancy ? "occupancy image" : (!pose ? "pose" : (!m ? "map description" : "map_out"))));
    size_t cells = 0;
    int rc = image_args(g->nx, g->ny, frames, kFusionWho, cells);
    if (rc) return rc;
    if (g->flags != 0) return fail(PWPP_E_ARG, "grid flags %d: the fusion's frame grid takes 0", g->flags);
    MapPlan plan;
    PwppFusionParams P;
    if ((rc = fusion_args(g, frames, pose, n_poses, map_of_frame, m, n_maps, shift, map_in, map_out, map_occupancy, plan, P))) return rc;
    if ((rc = mem_args(mem, kFusionWho))) return rc;
    Staging st(h, h->d_clusters, mem, kClusterAlign);
    const int s_occ = st.add_bytes(cells, occupancy, Staging::kIn);
    const FusionSections s = fusion_sections(st, plan, s_occ, map_in, map_out, map_occupancy);
    return run_on_image(h, st, [&] { return fusion_launch(h, st, s, plan, P, frames); });
}

// pwpp_visibility_obstacles and pwpp_fuse_grid on its bytes (run_on_visibility).
int pwpp_fuse_obstacles(pwpp_handle *h, const pwpp_ground_grid *g, float h_min, float h_max, int min_count, const double *origin_xy, int n_origins,
                        int max_range, int frame_first, int frames, int mem, const double *pose, int n_poses, const int32_t *map_of_frame,
                        const pwpp_fusion_map *m, int n_maps, const int32_t *shift, const int16_t *map_in, int16_t *map_out, int8_t *map_occupancy,
                        int8_t *occupancy) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!g || !origin_xy || !pose || !m || !map_out)
        return fail(PWPP_E_ARG, "null %s", !g ? "grid" : (!origin_xy ? "origin" : (!pose ? "pose" : (!m ? "map description" : "map_out"))));
    std::vector<int32_t> org;
    MapPlan plan;
    PwppFusionParams P;
    int rc = visibility_first_args(g, h_min, h_max, min_count, origin_xy, n_origins, max_range, frames, org);
    if (rc || (rc = fusion_args(g, frames, pose, n_poses, map_of_frame, m, n_maps, shift, map_in, map_out, map_occupancy, plan, P))) return rc;
    size_t cells = 0;
    if ((rc = ground_grid_args(h, g, frame_first, frames, mem, cells))) return rc;
    return run_on_visibility(h, g, h_min, h_max, min_count, org, max_range, frame_first, frames, mem, cells, occupancy, [&](Staging &st, int s_occ) {
        const FusionSections s = fusion_sections(st, plan, s_occ, map_in, map_out, map_occupancy);
        return [&, s] { return fusion_launch(h, st, s, plan, P, frames); };
    });
}

// ---- scan match: the map's log-odds summed under a frame's occupied cells, for every candidate pose and whole-cell shift ----------
namespace {
static_assert(PWPP_OCC_OCCUPIED == PWPP_MATCH_OCCUPIED, "the kernel's occupied byte");
static_assert(sizeof(pwpp_match_best) == 24 && sizeof(PwppMatchKey) == 24 && alignof(pwpp_match_best) == 8, "pwpp_match_best is 24 bytes, 8-byte aligned");
static_assert(offsetof(pwpp_match_best, candidate) == offsetof(PwppMatchKey, candidate) && offsetof(pwpp_match_best, cells) == offsetof(PwppMatchKey, cells),
              "the kernels write pwpp_match_best rows");
constexpr const char *kMatchWho = "the scan match takes";

// What a checked call hands to the kernels besides its images: the geometry, the counts and the words to upload -- the candidates
// first (8-byte aligned at the section's start), then every frame's map, the rule of map_of_frame resolved.
struct MatchPlan {
    PwppMatchGeometry G;
    int n_sets = 0, n_candidates = 0, n_maps = 0, wx = 0, wy = 0;
    size_t map_cells = 0;    // NX * NY * n_maps
    size_t score_count = 0;  // frames * n_candidates * (2 wy + 1) * (2 wx + 1) where the caller wants the scores, else 0
    std::vector<uint32_t> words;
    size_t at_maps() const { return (size_t)n_sets * (size_t)n_candidates * 12; }
};

// What both entry points check of the map, the candidates, the window and the frames' maps, in the header's order, after the frame
// images' own checks (frames >= 1); fills the plan.  Touches no handle.
int match_args(const pwpp_ground_grid *g, int frames, const double *candidates, int n_sets, int n_candidates, const int32_t *map_of_frame,
               const pwpp_fusion_map *m, int n_maps, int wx, int wy, const int64_t *scores, MatchPlan &plan) {
    if (const int rc = map_grid_args(g, m, n_maps, kMatchWho, plan.map_cells)) return rc;
    if (n_candidates < 1 || n_candidates > PWPP_MATCH_MAX_CANDIDATES) return fail(PWPP_E_ARG, "%d candidates: 1 .. 256 expected", n_candidates);
    if (const int rc = per_frame_count_args(n_sets, frames, "candidate sets")) return rc;
    if (wx < 0 || wx > PWPP_MATCH_MAX_WINDOW || wy < 0 || wy > PWPP_MATCH_MAX_WINDOW)
        return fail(PWPP_E_ARG, "window wx %d, wy %d: 0 .. 64 cells expected", wx, wy);
    if ((int64_t)frames * (int64_t)n_candidates > ((int64_t)1 << 24))
        return fail(PWPP_E_ARG, "%d frames x %d candidates exceed 2^24", frames, n_candidates);
    const int64_t per_pair = (int64_t)(2 * wx + 1) * (int64_t)(2 * wy + 1);  // (<= 129^2; frames x candidates <= 2^24)
    if (scores && (int64_t)frames * (int64_t)n_candidates * per_pair > ((int64_t)1 << 31))
        return fail(PWPP_E_ARG, "%d frames x %d candidates x %lld shifts: the scores exceed 2^31 elements", frames, n_candidates, (long long)per_pair);
    const FrameMaps map_of{map_of_frame, n_maps};
    if (const int rc = map_of.args(frames)) return rc;

    plan.G = PwppMatchGeometry{m->x0, m->y0, m->cell, g->x0, g->y0, g->cell, m->nx, m->ny, g->nx, g->ny, 0.0};
    pwpp_fuse_reciprocal(m->cell, plan.G.inv_CELL);
    plan.n_sets = n_sets, plan.n_candidates = n_candidates, plan.n_maps = n_maps, plan.wx = wx, plan.wy = wy;
    plan.score_count = scores ? (size_t)frames * (size_t)n_candidates * (size_t)per_pair : 0;
    try {
        plan.words.assign(plan.at_maps() + (size_t)frames, 0u);
    } catch (const std::bad_alloc &) {
        return fail(PWPP_E_NOMEM, "no host memory for %d candidate sets of %d and %d frames", n_sets, n_candidates, frames);
    }
    std::memcpy(plan.words.data(), candidates, (size_t)n_sets * (size_t)n_candidates * 6 * sizeof(double));
    for (int i = 0; i < frames; ++i) plan.words[plan.at_maps() + (size_t)i] = (uint32_t)map_of(i);
    return PWPP_OK;
}

// (after mem: what PWPP_MEM_DEVICE asks of the result arrays; the map is 2-byte aligned and the bytes byte aligned, no more)
int match_alignment_args(int mem, const void *best, const void *scores) { return alignment_args(mem, {{best, 7u, "best rows"}, {scores, 7u, "scores"}}); }

// (the plan's words, which move into the staging, and the kernels' working words first -- cell list, counts and workgroup bests are kKept like every operator's
// work words: theirs alone, in the buffer whatever the memory kind; `occ` is the frame bytes' section: the caller's, or the visibility's)
struct MatchSections {
    int up, work, occ, map, best, scores;
};
MatchSections match_sections(Staging &st, MatchPlan &plan, int frames, int s_occ, const int16_t *map, pwpp_match_best *best, int64_t *scores) {
    MatchSections s;
    s.up = st.add_upload(std::move(plan.words));
    s.work = st.add(pwpp_match_work_words(plan.G.nx, plan.G.ny, frames, plan.n_candidates, plan.wx, plan.wy), nullptr, Staging::kKept);
    s.occ = s_occ;
    s.map = st.add((plan.map_cells + 1) / 2, map, Staging::kIn, plan.map_cells * sizeof(int16_t));
    s.best = st.add((size_t)frames * (sizeof(pwpp_match_best) / 4), best, Staging::kOut);
    s.scores = st.add(plan.score_count * 2, scores, Staging::kOut);
    return s;
}
int match_launch(pwpp_handle *h, const Staging &st, const MatchSections &s, const MatchPlan &plan, int frames) {
    return pwpp_launch_match_grid(&plan.G, frames, st.dev<const int8_t>(s.occ), st.dev<const double>(s.up), plan.n_sets, plan.n_candidates,
                                  st.dev<const int32_t>(s.up) + plan.at_maps(), plan.n_maps, st.dev<const int16_t>(s.map), plan.wx, plan.wy,
                                  st.dev<void>(s.best), st.dev<int64_t>(s.scores), st.dev<uint32_t>(s.work), h->match_path, h->stream);
}
}  // namespace

int pwpp_match_grid(pwpp_handle *h, const pwpp_ground_grid *g, int frames, int mem, const int8_t *occupancy, const double *candidates, int n_sets,
                    int n_candidates, const int32_t *map_of_frame, const pwpp_fusion_map *m, int n_maps, const int16_t *map, int wx, int wy,
                    pwpp_match_best *best, int64_t *scores) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!g || !occupancy || !candidates || !m || !map || !best)
        return fail(PWPP_E_ARG, "null %s",
                    !g ? "grid" : (!occupancy ? "occupancy image" : (!candidates ? "candidates" : (!m ? "map description" : (!map ? "map" : "best rows")))));
    size_t cells = 0;
    int rc = image_args(g->nx, g->ny, frames, kMatchWho, cells);
    if (rc) return rc;
    if (g->flags != 0) return fail(PWPP_E_ARG, "grid flags %d: the scan match's frame grid takes 0", g->flags);
    MatchPlan plan;
    if ((rc = match_args(g, frames, candidates, n_sets, n_candidates, map_of_frame, m, n_maps, wx, wy, scores, plan))) return rc;
    if ((rc = mem_args(mem, kMatchWho))) return rc;
    if ((rc = match_alignment_args(mem, best, scores))) return rc;
    Staging st(h, h->d_clusters, mem, kClusterAlign);
    const int s_occ = st.add_bytes(cells, occupancy, Staging::kIn);
    const MatchSections s = match_sections(st, plan, frames, s_occ, map, best, scores);
    return run_on_image(h, st, [&] { return match_launch(h, st, s, plan, frames); });
}

// pwpp_visibility_obstacles and pwpp_match_grid on its bytes (run_on_visibility).
int pwpp_match_obstacles(pwpp_handle *h, const pwpp_ground_grid *g, float h_min, float h_max, int min_count, const double *origin_xy, int n_origins,
                         int max_range, int frame_first, int frames, int mem, const double *candidates, int n_sets, int n_candidates,
                         const int32_t *map_of_frame, const pwpp_fusion_map *m, int n_maps, const int16_t *map, int wx, int wy, pwpp_match_best *best,
                         int64_t *scores, int8_t *occupancy) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!g || !origin_xy || !candidates || !m || !map || !best)
        return fail(PWPP_E_ARG, "null %s",
                    !g ? "grid" : (!origin_xy ? "origin" : (!candidates ? "candidates" : (!m ? "map description" : (!map ? "map" : "best rows")))));
    std::vector<int32_t> org;
    MatchPlan plan;
    int rc = visibility_first_args(g, h_min, h_max, min_count, origin_xy, n_origins, max_range, frames, org);
    if (rc || (rc = match_args(g, frames, candidates, n_sets, n_candidates, map_of_frame, m, n_maps, wx, wy, scores, plan))) return rc;
    size_t cells = 0;
    if ((rc = ground_grid_args(h, g, frame_first, frames, mem, cells))) return rc;
    if ((rc = match_alignment_args(mem, best, scores))) return rc;
    return run_on_visibility(h, g, h_min, h_max, min_count, org, max_range, frame_first, frames, mem, cells, occupancy, [&](Staging &st, int s_occ) {
        const MatchSections s = match_sections(st, plan, frames, s_occ, map, best, scores);
        return [&, s] { return match_launch(h, st, s, plan, frames); };
    });
}

// Host only: the candidate moved by the winning shift, with the rounding of pwpp_match.h.
int pwpp_match_pose(const double candidate[6], double CELL, int sx, int sy, double out[6]) {
    if (!candidate || !out) return fail(PWPP_E_ARG, "null %s", candidate ? "output pose" : "candidate");
    pwpp_match_shifted_pose(candidate, CELL, sx, sy, out);
    return PWPP_OK;
}

// ---- elevation fusion: per-frame ground heights, under a pose and a height offset per frame, into persistent (sum, n) maps ---------
namespace {
static_assert(sizeof(pwpp_height_map) == 40, "pwpp_height_map is 40 bytes");
constexpr const char *kElevationWho = "the elevation fusion takes";

// What both entry points check of the map, the poses, the frame lists, the shifts, the inputs and the overlaps, in the header's
// order, after the frame images' own checks (frames >= 1); fills the plan (one more double for every pose: z_offset, zeros
// without it) and the parameters.  Touches no handle.
int height_args(const pwpp_ground_grid *g, int frames, const double *pose, const double *z_offset, int n_poses, const int32_t *map_of_frame,
                const pwpp_height_map *m, int n_maps, const int32_t *shift, const int32_t *sum_in, const int16_t *n_in, const int32_t *sum_out,
                const int16_t *n_out, const float *mean, MapPlan &plan, PwppElevationParams &P) {
    if (const int rc = map_grid_args(g, m, n_maps, kElevationWho, plan.map_cells)) return rc;
    if (m->n_max < 1 || m->n_max > PWPP_ELEV_MAX_N) return fail(PWPP_E_ARG, "n_max %d: 1 .. 1023 expected", m->n_max);
    if (m->pad_ != 0) return fail(PWPP_E_ARG, "pad_ %d of the height map: 0 expected", m->pad_);
    if (const int rc = map_plan_args(g, m, frames, n_poses, 1, map_of_frame, n_maps, shift, plan)) return rc;
    if (!sum_in != !n_in) return fail(PWPP_E_ARG, "null %s with a %s: both or neither expected", sum_in ? "n_in" : "sum_in", sum_in ? "sum_in" : "n_in");
    const size_t words = plan.map_cells * 4, halves = plan.map_cells * 2;  // (bytes; sum_out == sum_in, n_out == n_in: in place)
    const int rc = range_args({{sum_in, words, "sum_in"}, {n_in, halves, "n_in"}, {sum_out, words, "sum_out"}, {n_out, halves, "n_out"}, {mean, words, "mean"}},
                              {{0, 2}, {1, 3}}, plan.moved);
    P = pwpp_elev_magic(m->n_max);
    return rc ? rc : map_plan_words(frames, pose, z_offset, map_of_frame, shift, plan);
}

// (after mem: what PWPP_MEM_DEVICE asks of the arrays -- words 4-byte, counts 2-byte aligned, no more; named in this order)
int height_alignment_args(int mem, const void *height, const void *sum_in, const void *n_in, const void *sum_out, const void *n_out, const void *mean) {
    return alignment_args(mem, {{height, 3u, "height images"}, {mean, 3u, "mean"}, {sum_in, 3u, "sums"}, {sum_out, 3u, "sums"}, {n_in, 1u, "counts"}, {n_out, 1u, "counts"}});
}

// (the plan's words first: they move into the staging; `height` is the frame images' section: the caller's, or the ground raster's)
struct HeightSections {
    int up, height, sum_in, n_in, sum_out, n_out, mean;
};
HeightSections height_sections(Staging &st, MapPlan &plan, int s_height, const int32_t *sum_in, const int16_t *n_in, int32_t *sum_out, int16_t *n_out,
                               float *mean) {
    HeightSections s;
    const size_t n_words = (plan.map_cells + 1) / 2, n_bytes = plan.map_cells * sizeof(int16_t);
    s.up = st.add_upload(std::move(plan.words));
    s.height = s_height;
    s.sum_in = st.add(sum_in ? plan.map_cells : 0, sum_in, Staging::kIn);
    s.n_in = st.add(n_in ? n_words : 0, n_in, Staging::kIn, n_in ? n_bytes : 0);
    s.sum_out = st.add(plan.map_cells, sum_out, Staging::kOut);
    s.n_out = st.add(n_words, n_out, Staging::kOut, n_bytes);
    s.mean = st.add(mean ? plan.map_cells : 0, mean, Staging::kOut);
    return s;
}
int height_launch(pwpp_handle *h, const Staging &st, const HeightSections &s, const MapPlan &plan, const PwppElevationParams &P, int frames) {
    const int32_t *words = st.dev<const int32_t>(s.up);
    return pwpp_launch_fuse_height(&plan.G, &P, frames, st.dev<const float>(s.height), st.dev<const double>(s.up),
                                   reinterpret_cast<const double *>(words + plan.at_per_pose()), plan.n_poses, plan.n_maps, words + plan.at_begin(),
                                   words + plan.at_list(), plan.listed, plan.shifted ? words + plan.at_shift() : nullptr, st.dev<const int32_t>(s.sum_in),
                                   st.dev<const int16_t>(s.n_in), st.dev<int32_t>(s.sum_out), st.dev<int16_t>(s.n_out), st.dev<float>(s.mean),
                                   h->elevation_path, h->stream);
}
const char *height_null(const void *g, const void *first, const char *first_name, const void *pose, const void *m, const void *sum_out, const void *n_out) {
    return !g ? "grid" : (!first ? first_name : (!pose ? "pose" : (!m ? "map description" : (!sum_out ? "sum_out" : (!n_out ? "n_out" : nullptr)))));
}
}  // namespace

int pwpp_fuse_height_grid(pwpp_handle *h, const pwpp_ground_grid *g, int frames, int mem, const float *height, const double *pose, const double *z_offset,
                          int n_poses, const int32_t *map_of_frame, const pwpp_height_map *m, int n_maps, const int32_t *shift, const int32_t *sum_in,
                          const int16_t *n_in, int32_t *sum_out, int16_t *n_out, float *mean) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (const char *what = height_null(g, height, "height images", pose, m, sum_out, n_out)) return fail(PWPP_E_ARG, "null %s", what);
    size_t cells = 0;
    int rc = image_args(g->nx, g->ny, frames, kElevationWho, cells);
    if (rc) return rc;
    if (g->flags != 0) return fail(PWPP_E_ARG, "grid flags %d: the elevation fusion's frame grid takes 0", g->flags);
    MapPlan plan;
    PwppElevationParams P;
    if ((rc = height_args(g, frames, pose, z_offset, n_poses, map_of_frame, m, n_maps, shift, sum_in, n_in, sum_out, n_out, mean, plan, P))) return rc;
    if ((rc = mem_args(mem, kElevationWho))) return rc;
    if ((rc = height_alignment_args(mem, height, sum_in, n_in, sum_out, n_out, mean))) return rc;
    Staging st(h, h->d_clusters, mem, kClusterAlign);
    const int s_height = st.add(cells, height, Staging::kIn);
    const HeightSections s = height_sections(st, plan, s_height, sum_in, n_in, sum_out, n_out, mean);
    return run_on_image(h, st, [&] { return height_launch(h, st, s, plan, P, frames); });
}

// pwpp_rasterize_ground into a section of the cluster buffer (or the caller's images) and pwpp_fuse_height_grid on it, one enqueued sequence.
int pwpp_fuse_ground(pwpp_handle *h, const pwpp_ground_grid *g, int frame_first, int frames, int mem, const double *pose, const double *z_offset, int n_poses,
                     const int32_t *map_of_frame, const pwpp_height_map *m, int n_maps, const int32_t *shift, const int32_t *sum_in, const int16_t *n_in,
                     int32_t *sum_out, int16_t *n_out, float *mean, float *height) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (const char *what = height_null(g, g, "", pose, m, sum_out, n_out)) return fail(PWPP_E_ARG, "null %s", what);
    int rc = ground_first_args(g, frames, kElevationWho);
    if (rc) return rc;
    MapPlan plan;
    PwppElevationParams P;
    if ((rc = height_args(g, frames, pose, z_offset, n_poses, map_of_frame, m, n_maps, shift, sum_in, n_in, sum_out, n_out, mean, plan, P))) return rc;
    size_t cells = 0;
    if ((rc = ground_grid_args(h, g, frame_first, frames, mem, cells))) return rc;
    if ((rc = height_alignment_args(mem, height, sum_in, n_in, sum_out, n_out, mean))) return rc;
    Staging st(h, h->d_clusters, mem, kClusterAlign);
    const int s_height = add_image(st, cells, height, true);
    const HeightSections s = height_sections(st, plan, s_height, sum_in, n_in, sum_out, n_out, mean);
    return run_on_ground(h, st, g, frame_first, frames, s_height, -1, [&] { return height_launch(h, st, s, plan, P, frames); });
}

// ---- terrain analysis: step, slope, roughness and cost of the window around every cell of a height image --------------------------
namespace {
static_assert(sizeof(pwpp_terrain_params) == 24, "pwpp_terrain_params is 24 bytes");
constexpr const char *kTerrainWho = "the terrain analysis takes";

// What both entry points check of the parameters and the overlaps, in the header's order, after the image's own checks; `cells`:
// nx * ny * frames; fills the rule.  Touches no handle.
int terrain_args(const pwpp_terrain_params *p, double cell, size_t cells, const float *height, const float *step, const float *slope, const float *rough,
                 const uint8_t *count, const int8_t *cost, PwppTerrainRule &rule) {
    if (p->radius < 1 || p->radius > PWPP_TERRAIN_MAX_R) return fail(PWPP_E_ARG, "radius %d: 1 .. 4 expected", p->radius);
    const int window = (2 * p->radius + 1) * (2 * p->radius + 1);
    if (p->min_known < 1 || p->min_known > window) return fail(PWPP_E_ARG, "min_known %d: 1 .. %d expected with radius %d", p->min_known, window, p->radius);
    if (!(p->step_max > 0.0f) || !(p->slope_max > 0.0f) || !(p->rough_max > 0.0f))
        return fail(PWPP_E_ARG, "limits %g (step), %g (slope), %g (rough): each > 0 expected, +inf allowed, not a NaN", (double)p->step_max,
                    (double)p->slope_max, (double)p->rough_max);
    if (p->pad_ != 0) return fail(PWPP_E_ARG, "pad_ %d of the terrain parameters: 0 expected", p->pad_);
    rule = PwppTerrainRule{p->radius, p->min_known, p->step_max, p->slope_max, p->rough_max, 1024.0 * cell};
    const size_t floats = cells * 4;  // (bytes)
    return range_args({{height, floats, "height"}, {step, floats, "step"}, {slope, floats, "slope"}, {rough, floats, "rough"}, {count, cells, "count"}, {cost, cells, "cost"}},
                      {}, false);
}

// (after mem: what PWPP_MEM_DEVICE asks of the arrays -- floats 4-byte aligned, bytes anywhere)
int terrain_alignment_args(int mem, const void *height, const void *step, const void *slope, const void *rough) {
    return alignment_args(mem, {{height, 3u, "height images"}, {step, 3u, "step"}, {slope, 3u, "slope"}, {rough, 3u, "rough"}});
}

// (`height` is the height images' section: the caller's, or the ground raster's)
struct TerrainSections {
    int height, step, slope, rough, count, cost;
};
TerrainSections terrain_sections(Staging &st, size_t cells, int s_height, float *step, float *slope, float *rough, uint8_t *count, int8_t *cost) {
    TerrainSections s;
    s.height = s_height;
    s.step = st.add(step ? cells : 0, step, Staging::kOut);
    s.slope = st.add(slope ? cells : 0, slope, Staging::kOut);
    s.rough = st.add(rough ? cells : 0, rough, Staging::kOut);
    s.count = st.add_bytes(cells, count, Staging::kOut);
    s.cost = st.add_bytes(cells, cost, Staging::kOut);
    return s;
}
// The analysis as a stage of a longer chain, for its cost bytes alone (the reach and the costmap on the ground raster): the raster's height kept in the
// buffer, one section without words for the four outputs nobody asks for -- null pointers -- and the cost: the caller's where given, else kept too.
TerrainSections terrain_cost_sections(Staging &st, size_t cells, int8_t *cost) {
    TerrainSections s;
    s.height = add_image(st, cells, nullptr, true);
    s.step = s.slope = s.rough = s.count = st.add(0, nullptr, Staging::kOut);
    s.cost = st.add_bytes(cells, cost, cost ? Staging::kOut : Staging::kKept);
    return s;
}
int terrain_launch(pwpp_handle *h, const Staging &st, const TerrainSections &s, const PwppTerrainRule &rule, int nx, int ny, int frames) {
    return pwpp_launch_terrain(&rule, nx, ny, frames, st.dev<const float>(s.height), st.dev<float>(s.step), st.dev<float>(s.slope), st.dev<float>(s.rough),
                               st.dev<uint8_t>(s.count), st.dev<int8_t>(s.cost), h->terrain_path, h->stream);
}
}  // namespace

int pwpp_terrain_grid(pwpp_handle *h, int nx, int ny, int frames, double cell, int mem, const float *height, const pwpp_terrain_params *p, float *step,
                      float *slope, float *rough, uint8_t *count, int8_t *cost) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!height || !p) return fail(PWPP_E_ARG, "null %s", !height ? "height images" : "terrain parameters");
    if (!step && !slope && !rough && !count && !cost) return fail(PWPP_E_ARG, "null outputs: at least one of step, slope, rough, count and cost expected");
    size_t cells = 0;
    int rc = image_args(nx, ny, frames, kTerrainWho, cells);
    if (rc) return rc;
    if (!(cell > 0.0) || !std::isfinite(cell)) return fail(PWPP_E_ARG, "cell size %g: finite and positive expected", cell);
    PwppTerrainRule rule;
    if ((rc = terrain_args(p, cell, cells, height, step, slope, rough, count, cost, rule))) return rc;
    if ((rc = mem_args(mem, kTerrainWho))) return rc;
    if ((rc = terrain_alignment_args(mem, height, step, slope, rough))) return rc;
    Staging st(h, h->d_clusters, mem, kClusterAlign);
    const int s_height = st.add(cells, height, Staging::kIn);
    const TerrainSections s = terrain_sections(st, cells, s_height, step, slope, rough, count, cost);
    return run_on_image(h, st, [&] { return terrain_launch(h, st, s, rule, nx, ny, frames); });
}

// pwpp_rasterize_ground into a section of the cluster buffer (or the caller's images) and pwpp_terrain_grid on it, one enqueued sequence.
int pwpp_terrain_ground(pwpp_handle *h, const pwpp_ground_grid *g, int frame_first, int frames, int mem, const pwpp_terrain_params *p, float *step,
                        float *slope, float *rough, uint8_t *count, int8_t *cost, float *height) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!g || !p) return fail(PWPP_E_ARG, "null %s", !g ? "grid" : "terrain parameters");
    if (!step && !slope && !rough && !count && !cost) return fail(PWPP_E_ARG, "null outputs: at least one of step, slope, rough, count and cost expected");
    int rc = ground_first_args(g, frames, kTerrainWho);
    if (rc) return rc;
    PwppTerrainRule rule;
    // (the byte ranges of the overlap check: sides <= 2^15 and frames < 2^31, the product fits 64 bits; ground_grid_args names one beyond 2^31)
    size_t cells = (size_t)g->nx * (size_t)g->ny * (size_t)frames;
    if ((rc = terrain_args(p, g->cell, cells, height, step, slope, rough, count, cost, rule))) return rc;
    if ((rc = ground_grid_args(h, g, frame_first, frames, mem, cells))) return rc;
    if ((rc = terrain_alignment_args(mem, height, step, slope, rough))) return rc;
    Staging st(h, h->d_clusters, mem, kClusterAlign);
    const int s_height = add_image(st, cells, height, true);
    const TerrainSections s = terrain_sections(st, cells, s_height, step, slope, rough, count, cost);
    return run_on_ground(h, st, g, frame_first, frames, s_height, -1, [&] { return terrain_launch(h, st, s, rule, g->nx, g->ny, frames); });
}

// ---- cost to reach: the cheapest sum of steps from the frame's source to every cell of a cost image, and the neighbour it comes through ----
namespace {
static_assert(sizeof(pwpp_reach_params) == 24, "pwpp_reach_params is 24 bytes");
static_assert(PWPP_REACH_NONE == (int32_t)PWPP_REACH_UNREACHED && PWPP_DIST_BEYOND == PWPP_REACH_DIST_BEYOND, "the kernels' values");
constexpr const char *kReachWho = "the reach takes";

// What both entry points check of the parameters and the range, in the header's order, after the image's own checks; fills the
// rule.  Touches no handle.  (`with_range` false: the footprints, which sum nothing over the image.)
int reach_param_args(const pwpp_reach_params *p, int nx, int ny, bool with_dist2, PwppReachRule &rule, bool with_range = true) {
    if (p->base < 1 || p->base > 255) return fail(PWPP_E_ARG, "base %d: 1 .. 255 expected", p->base);
    if (p->lethal < 1 || p->lethal > 101) return fail(PWPP_E_ARG, "lethal %d: 1 .. 101 expected (101: no value is lethal)", p->lethal);
    if (p->unknown < -1 || p->unknown > 100) return fail(PWPP_E_ARG, "unknown %d: -1 (impassable) .. 100 expected", p->unknown);
    if (with_dist2 && p->clearance2 < 0) return fail(PWPP_E_ARG, "clearance2 %d: at least 0 expected", p->clearance2);
    if (p->max_reach < 0) return fail(PWPP_E_ARG, "max_reach %d: 0 (unlimited) or more expected", p->max_reach);
    if (p->pad_ != 0) return fail(PWPP_E_ARG, "pad_ %d of the reach parameters: 0 expected", p->pad_);
    int64_t worst = 0;
    if (with_range && !pwpp_reach_range_ok(p->base, nx, ny, worst))
        return fail(PWPP_E_ARG, "14 * (base + 100) * (%d * %d - 1) = %lld with base %d exceeds 2^31 - 2: a reach would not fit 32 bits", nx, ny,
                    (long long)worst, p->base);
    rule = PwppReachRule{p->base, p->lethal, p->unknown, with_dist2 ? p->clearance2 : 0, p->max_reach, with_dist2 ? 1 : 0};
    return PWPP_OK;
}

// What the entry points on a caller's cost image check first, in the header's order, after their null pointers: the image's shape
// (`cells`: nx * ny * frames), the parameters, the number of sources and the source cells.  Touches no handle.
int reach_image_args(int nx, int ny, int frames, const int32_t *dist2, const pwpp_reach_params *p, const int32_t *source, int n_sources, size_t &cells,
                     PwppReachRule &rule) {
    int rc = image_args(nx, ny, frames, kReachWho, cells);
    if (rc) return rc;
    if ((rc = reach_param_args(p, nx, ny, dist2 != nullptr, rule))) return rc;
    if ((rc = per_frame_count_args(n_sources, frames, "sources"))) return rc;
    return cells_inside_args(source, n_sources, nx, ny, "source");
}

// What becomes of the field (reach, from) of a call: written for the caller (from where asked for); ... and kept in the buffer where the caller gives
// no pointer -- the routes read it there; or not computed at all: the caller's `from` is read by the routes, and there is no working image, defect
// word or reach section.
enum class ReachField { kWritten, kKept, kRead };

// (the working image, the defect word and the sources first; `src`: the source cells, n_sources x {sx, sy}, checked; `cost` is the
// cost bytes' section: the caller's, or the terrain's.  In PWPP_MEM_HOST the defect word comes back with the images.)
struct ReachSections {
    int term, flag, src, cost, dist2, reach, from;
};
ReachSections reach_sections(Staging &st, int mem, int nx, int ny, int frames, size_t cells, int s_cost, const std::vector<int32_t> &src, const int32_t *dist2,
                             int32_t *reach, const int32_t *from, uint32_t *flag_host, ReachField field = ReachField::kWritten) {
    ReachSections s{};
    const bool computed = field != ReachField::kRead, keep = field == ReachField::kKept;
    if (computed) {
        s.term = st.add(pwpp_reach_work_words(nx, ny, frames), nullptr, Staging::kKept);
        s.flag = mem == PWPP_MEM_HOST ? st.add(1, flag_host, Staging::kOut) : st.add(1, nullptr, Staging::kKept);
    }
    s.src = frame_cells_section(st, src);
    s.cost = s_cost;
    s.dist2 = st.add(dist2 ? cells : 0, dist2, Staging::kIn);
    if (computed) {
        s.reach = st.add(cells, reach, keep && !reach ? Staging::kKept : Staging::kOut);
        s.from = st.add(from || keep ? cells : 0, from, keep && !from ? Staging::kKept : Staging::kOut);
    } else {
        s.from = st.add(cells, from, Staging::kIn);
    }
    return s;
}
// (one source travels as an argument; one per frame lies in its section)
int reach_launch(pwpp_handle *h, const Staging &st, const ReachSections &s, const PwppReachRule &rule, int nx, int ny, int frames, const std::vector<int32_t> &src) {
    return pwpp_launch_reach(&rule, nx, ny, frames, st.dev<const int8_t>(s.cost), rule.use_dist2 ? st.dev<const int32_t>(s.dist2) : nullptr, src[0], src[1],
                             src.size() > 2 ? st.dev<const int32_t>(s.src) : nullptr, st.dev<int32_t>(s.reach), st.dev<int32_t>(s.from),
                             st.dev<uint16_t>(s.term), st.dev<uint32_t>(s.flag), h->reach_path, h->stream);
}
// (PWPP_MEM_HOST, after the images came back: a kernel that met a loop bound)
int reach_defect(int rc, uint32_t flag_host) {
    if (rc == PWPP_OK && flag_host != 0) return fail(PWPP_E_HIP, "internal error: a reach kernel met the bound of its sweeps (a defect, not an input)");
    return rc;
}
}  // namespace

int pwpp_reach_grid(pwpp_handle *h, int nx, int ny, int frames, int mem, const int8_t *cost, const int32_t *dist2, const pwpp_reach_params *p,
                    const int32_t *source, int n_sources, int32_t *reach, int32_t *from) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!cost || !p || !source || !reach)
        return fail(PWPP_E_ARG, "null %s", !cost ? "cost image" : (!p ? "reach parameters" : (!source ? "source" : "reach image")));
    size_t cells = 0;
    PwppReachRule rule;
    int rc = reach_image_args(nx, ny, frames, dist2, p, source, n_sources, cells, rule);
    if (rc) return rc;
    if ((rc = range_args({{cost, cells, "cost"}, {dist2, cells * 4, "dist2"}, {reach, cells * 4, "reach"}, {from, cells * 4, "from"}}, {}, false))) return rc;
    if ((rc = mem_args(mem, kReachWho))) return rc;
    if ((rc = alignment_args(mem, {{dist2, 3u, "dist2 image"}, {reach, 3u, "reach image"}, {from, 3u, "from image"}}))) return rc;
    const std::vector<int32_t> src(source, source + 2 * (size_t)n_sources);
    uint32_t flag_host = 0;
    Staging st(h, h->d_clusters, mem, kClusterAlign);
    const int s_cost = st.add_bytes(cells, cost, Staging::kIn);
    const ReachSections s = reach_sections(st, mem, nx, ny, frames, cells, s_cost, src, dist2, reach, from, &flag_host);
    return reach_defect(run_on_image(h, st, [&] { return reach_launch(h, st, s, rule, nx, ny, frames, src); }), flag_host);
}

// pwpp_rasterize_ground into a section of the cluster buffer, pwpp_terrain_grid for its cost bytes alone (kept there too unless the caller asks for
// them) and pwpp_reach_grid on those, one enqueued sequence.
int pwpp_reach_ground(pwpp_handle *h, const pwpp_ground_grid *g, int frame_first, int frames, int mem, const pwpp_terrain_params *tp, const pwpp_reach_params *p,
                      const double *source_xy, int n_sources, int32_t *reach, int32_t *from, int8_t *cost) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!g || !tp || !p || !source_xy || !reach)
        return fail(PWPP_E_ARG, "null %s", !g ? "grid" : (!tp ? "terrain parameters" : (!p ? "reach parameters" : (!source_xy ? "source" : "reach image"))));
    int rc = ground_first_args(g, frames, kReachWho);
    if (rc) return rc;
    PwppTerrainRule terrain_rule;
    PwppReachRule rule;
    size_t cells = (size_t)g->nx * (size_t)g->ny * (size_t)frames;  // (as in pwpp_terrain_ground: fits 64 bits; ground_grid_args names one beyond 2^31)
    if ((rc = terrain_args(tp, g->cell, cells, nullptr, nullptr, nullptr, nullptr, nullptr, cost, terrain_rule))) return rc;
    if ((rc = reach_param_args(p, g->nx, g->ny, false, rule))) return rc;
    if ((rc = grid_geometry_args(g))) return rc;  // (the sources need the grid)
    if ((rc = per_frame_count_args(n_sources, frames, "sources"))) return rc;
    std::vector<int32_t> src;
    if ((rc = frame_cells_of(g, source_xy, n_sources, "source", src))) return rc;
    if ((rc = range_args({{cost, cells, "cost"}, {reach, cells * 4, "reach"}, {from, cells * 4, "from"}}, {}, false))) return rc;
    if ((rc = ground_grid_args(h, g, frame_first, frames, mem, cells))) return rc;
    if ((rc = alignment_args(mem, {{reach, 3u, "reach image"}, {from, 3u, "from image"}}))) return rc;
    uint32_t flag_host = 0;
    Staging st(h, h->d_clusters, mem, kClusterAlign);
    const TerrainSections t = terrain_cost_sections(st, cells, cost);
    const ReachSections s = reach_sections(st, mem, g->nx, g->ny, frames, cells, t.cost, src, nullptr, reach, from, &flag_host);
    return reach_defect(run_on_ground(h, st, g, frame_first, frames, t.height, -1,
                                      [&] {
                                          const int lrc = terrain_launch(h, st, t, terrain_rule, g->nx, g->ny, frames);
                                          return lrc != 0 ? lrc : reach_launch(h, st, s, rule, g->nx, g->ny, frames, src);
                                      }),
                        flag_host);
}

// The raster's cell rule for one position, as the origins and sources in metres go through it (frame_cells_of): for a caller
// who has a position in metres and a call that takes cells.  Reads the grid's origin, cell size and sides alone; no handle.
int pwpp_grid_cell_of(const pwpp_ground_grid *g, double x, double y, int32_t *ix, int32_t *iy) {
    if (!g || !ix || !iy) return fail(PWPP_E_ARG, "null %s", !g ? "grid" : "cell");
    if (const int rc = grid_geometry_args(g)) return rc;
    const double xy[2] = {x, y};
    std::vector<int32_t> cell;
    if (const int rc = frame_cells_of(g, xy, 1, "position", cell)) return rc;
    *ix = cell[0], *iy = cell[1];
    return PWPP_OK;
}

// ---- routes: the from chain of the reach field walked, summarised and shortcut for every (frame, start) ----
namespace {
static_assert(sizeof(pwpp_route_params) == 16 && sizeof(pwpp_route) == 32 && sizeof(PwppRouteRow) == 32 && sizeof(PwppRouteRule) == 16, "the rows and the rule as the kernels see them");
static_assert(PWPP_ROUTE_OK == PWPP_ROUTE_STATUS_OK && PWPP_ROUTE_NONE == PWPP_ROUTE_STATUS_NONE && PWPP_ROUTE_BROKEN == PWPP_ROUTE_STATUS_BROKEN, "the kernels' values");

// What both entry points check of the route's own arguments, in the header's order, after the reach's; fills the rule and `st`, the
// start cells n_start_sets x n_starts x {x, y}.  Touches no handle.
int route_args(const pwpp_route_params *q, int nx, int ny, int frames, const int32_t *start, int n_start_sets, int n_starts, const int32_t *cells,
               const int32_t *waypoints, PwppRouteRule &rule, std::vector<uint32_t> &st) {
    if (q->max_cells < 0) return fail(PWPP_E_ARG, "max_cells %d: 0 (no cell list) or more expected", q->max_cells);
    if (q->max_waypoints < 0) return fail(PWPP_E_ARG, "max_waypoints %d: 0 (no shortcut search) or more expected", q->max_waypoints);
    if (q->look < 1 || q->look > PWPP_ROUTE_MAX_LOOK) return fail(PWPP_E_ARG, "look %d: 1 .. %d expected", q->look, PWPP_ROUTE_MAX_LOOK);
    if (q->line_cost < 0 || q->line_cost > 100) return fail(PWPP_E_ARG, "line_cost %d: 0 .. 100 expected", q->line_cost);
    if (const int rc = per_frame_count_args(n_start_sets, frames, "start sets")) return rc;
    if (n_starts < 1 || n_starts > PWPP_ROUTE_MAX_STARTS) return fail(PWPP_E_ARG, "%d starts: 1 .. %d expected", n_starts, PWPP_ROUTE_MAX_STARTS);
    const int64_t per_route = std::max<int64_t>(std::max(q->max_cells, q->max_waypoints), 1);
    if ((int64_t)frames * (int64_t)n_starts > (int64_t)INT32_MAX / per_route)
        return fail(PWPP_E_ARG, "%d frames x %d starts x %lld list entries exceed 2^31 - 1", frames, n_starts, (long long)per_route);
    for (int k = 0; k < n_start_sets; ++k)
        for (int i = 0; i < n_starts; ++i) {
            const int32_t *s = start + 2 * ((size_t)k * (size_t)n_starts + (size_t)i);
            if (s[0] < 0 || s[0] >= nx || s[1] < 0 || s[1] >= ny)
                return fail(PWPP_E_ARG, "start %d of set %d, cell (%d, %d), lies outside the %d x %d cells", i, k, s[0], s[1], nx, ny);
        }
    if (q->max_cells > 0 && !cells) return fail(PWPP_E_ARG, "null cell lists with max_cells %d", q->max_cells);
    if (q->max_waypoints > 0 && !waypoints) return fail(PWPP_E_ARG, "null waypoint lists with max_waypoints %d", q->max_waypoints);
    rule = PwppRouteRule{q->max_cells, q->max_waypoints, q->look, q->line_cost};
    st.assign(start, start + 2 * (size_t)n_start_sets * (size_t)n_starts);
    return PWPP_OK;
}

// (the uploaded starts first, then the rows and the lists; a list without entries has no words and a null pointer)
struct RouteSections {
    int start, rows, cells, wps;
};
RouteSections route_sections(Staging &st, std::vector<uint32_t> &&starts, size_t routes, const PwppRouteRule &rule, pwpp_route *rows, int32_t *cells,
                             int32_t *waypoints) {
    RouteSections s;
    s.start = st.add_upload(std::move(starts));
    s.rows = st.add(routes * 8, rows, Staging::kOut);
    s.cells = st.add(routes * (size_t)rule.max_cells, rule.max_cells > 0 ? cells : nullptr, Staging::kOut);
    s.wps = st.add(routes * (size_t)rule.max_waypoints, rule.max_waypoints > 0 ? waypoints : nullptr, Staging::kOut);
    return s;
}
int route_launch(pwpp_handle *h, const Staging &st, const ReachSections &r, const RouteSections &s, const PwppReachRule &rule, const PwppRouteRule &route,
                 int nx, int ny, int frames, const std::vector<int32_t> &src, int n_start_sets, int n_starts) {
    return pwpp_launch_routes(&rule, &route, nx, ny, frames, st.dev<const int8_t>(r.cost), rule.use_dist2 ? st.dev<const int32_t>(r.dist2) : nullptr,
                              src[0], src[1], src.size() > 2 ? st.dev<const int32_t>(r.src) : nullptr,
                              st.dev<const int32_t>(r.from), st.dev<const int32_t>(s.start), n_start_sets, n_starts, st.dev<void>(s.rows), st.dev<int32_t>(s.cells),
                              st.dev<int32_t>(s.wps), h->route_path, h->stream);
}

// what both entry points check between the null pointers and the overlaps: what pwpp_reach_grid checks there, then the routes' own
int route_common_args(int nx, int ny, int frames, const int32_t *dist2, const pwpp_reach_params *p, const int32_t *source, int n_sources, const pwpp_route_params *q,
                      const int32_t *start, int n_start_sets, int n_starts, const int32_t *cells, const int32_t *waypoints, size_t &n_cells, PwppReachRule &rule,
                      PwppRouteRule &route, std::vector<uint32_t> &starts) {
    if (const int rc = reach_image_args(nx, ny, frames, dist2, p, source, n_sources, n_cells, rule)) return rc;
    return route_args(q, nx, ny, frames, start, n_start_sets, n_starts, cells, waypoints, route, starts);
}
}  // namespace

int pwpp_route_grid(pwpp_handle *h, int nx, int ny, int frames, int mem, const int8_t *cost, const int32_t *dist2, const pwpp_reach_params *p,
                    const int32_t *source, int n_sources, const int32_t *from, const int32_t *start, int n_start_sets, int n_starts, const pwpp_route_params *q,
                    pwpp_route *routes, int32_t *cells, int32_t *waypoints) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!cost || !p || !source || !from || !start || !q || !routes)
        return fail(PWPP_E_ARG, "null %s",
                    !cost ? "cost image" : (!p ? "reach parameters" : (!source ? "source" : (!from ? "from image" : (!start ? "start" : (!q ? "route parameters" : "routes"))))));
    size_t n_cells = 0;
    PwppReachRule rule;
    PwppRouteRule route;
    std::vector<uint32_t> starts;
    int rc = route_common_args(nx, ny, frames, dist2, p, source, n_sources, q, start, n_start_sets, n_starts, cells, waypoints, n_cells, rule, route, starts);
    if (rc) return rc;
    const size_t n_routes = (size_t)frames * (size_t)n_starts;
    if ((rc = range_args({{cost, n_cells, "cost"}, {dist2, n_cells * 4, "dist2"}, {from, n_cells * 4, "from"}, {routes, n_routes * 32, "routes"},
                          {route.max_cells > 0 ? cells : nullptr, n_routes * 4 * (size_t)route.max_cells, "cells"},
                          {route.max_waypoints > 0 ? waypoints : nullptr, n_routes * 4 * (size_t)route.max_waypoints, "waypoints"}}, {}, false)))
        return rc;
    if ((rc = mem_args(mem, "the routes take"))) return rc;
    if ((rc = alignment_args(mem, {{dist2, 3u, "dist2 image"}, {from, 3u, "from image"}, {routes, 3u, "routes"}, {route.max_cells > 0 ? cells : nullptr, 3u, "cell lists"},
                                   {route.max_waypoints > 0 ? waypoints : nullptr, 3u, "waypoint lists"}})))
        return rc;
    const std::vector<int32_t> src(source, source + 2 * (size_t)n_sources);
    Staging st(h, h->d_clusters, mem, kClusterAlign);
    const int s_cost = st.add_bytes(n_cells, cost, Staging::kIn);
    const ReachSections r = reach_sections(st, mem, nx, ny, frames, n_cells, s_cost, src, dist2, nullptr, from, nullptr, ReachField::kRead);
    const RouteSections s = route_sections(st, std::move(starts), n_routes, route, routes, cells, waypoints);
    return run_on_image(h, st, [&] { return route_launch(h, st, r, s, rule, route, nx, ny, frames, src, n_start_sets, n_starts); });
}

// pwpp_reach_grid -- reach and from kept in the cluster buffer unless the caller asks for them -- and pwpp_route_grid on its from, one enqueued
// sequence.
int pwpp_plan_grid(pwpp_handle *h, int nx, int ny, int frames, int mem, const int8_t *cost, const int32_t *dist2, const pwpp_reach_params *p,
                   const int32_t *source, int n_sources, const int32_t *start, int n_start_sets, int n_starts, const pwpp_route_params *q, pwpp_route *routes,
                   int32_t *cells, int32_t *waypoints, int32_t *reach, int32_t *from) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!cost || !p || !source || !start || !q || !routes)
        return fail(PWPP_E_ARG, "null %s", !cost ? "cost image" : (!p ? "reach parameters" : (!source ? "source" : (!start ? "start" : (!q ? "route parameters" : "routes")))));
    size_t n_cells = 0;
    PwppReachRule rule;
    PwppRouteRule route;
    std::vector<uint32_t> starts;
    int rc = route_common_args(nx, ny, frames, dist2, p, source, n_sources, q, start, n_start_sets, n_starts, cells, waypoints, n_cells, rule, route, starts);
    if (rc) return rc;
    const size_t n_routes = (size_t)frames * (size_t)n_starts;
    if ((rc = range_args({{cost, n_cells, "cost"}, {dist2, n_cells * 4, "dist2"}, {reach, n_cells * 4, "reach"}, {from, n_cells * 4, "from"}, {routes, n_routes * 32, "routes"},
                          {route.max_cells > 0 ? cells : nullptr, n_routes * 4 * (size_t)route.max_cells, "cells"},
                          {route.max_waypoints > 0 ? waypoints : nullptr, n_routes * 4 * (size_t)route.max_waypoints, "waypoints"}}, {}, false)))
        return rc;
    if ((rc = mem_args(mem, "the routes take"))) return rc;
    if ((rc = alignment_args(mem, {{dist2, 3u, "dist2 image"}, {reach, 3u, "reach image"}, {from, 3u, "from image"}, {routes, 3u, "routes"},
                                   {route.max_cells > 0 ? cells : nullptr, 3u, "cell lists"}, {route.max_waypoints > 0 ? waypoints : nullptr, 3u, "waypoint lists"}})))
        return rc;
    const std::vector<int32_t> src(source, source + 2 * (size_t)n_sources);
    uint32_t flag_host = 0;
    Staging st(h, h->d_clusters, mem, kClusterAlign);
    const int s_cost = st.add_bytes(n_cells, cost, Staging::kIn);
    const ReachSections r = reach_sections(st, mem, nx, ny, frames, n_cells, s_cost, src, dist2, reach, from, &flag_host, ReachField::kKept);
    const RouteSections s = route_sections(st, std::move(starts), n_routes, route, routes, cells, waypoints);
    return reach_defect(run_on_image(h, st,
                                     [&] {
                                         const int lrc = reach_launch(h, st, r, rule, nx, ny, frames, src);
                                         return lrc != 0 ? lrc : route_launch(h, st, r, s, rule, route, nx, ny, frames, src, n_start_sets, n_starts);
                                     }),
                        flag_host);
}

// ---- oriented vehicle footprint: the rectangle of every pose laid over the cost image, every trajectory's free prefix summed up ----
namespace {
static_assert(sizeof(pwpp_footprint_params) == 24 && sizeof(pwpp_footprint_pose_row) == 32 && sizeof(pwpp_footprint_traj_row) == 32 && sizeof(PwppFootPoseRow) == 32 &&
                  sizeof(PwppFootTrajRow) == 32 && sizeof(PwppFootPose) == 16 && sizeof(PwppFootRule) == 16,
              "the rows, the pose and the rule as the kernels see them");
static_assert(PWPP_FOOT_FREE == PWPP_FOOT_STATUS_FREE && PWPP_FOOT_HIT == PWPP_FOOT_STATUS_HIT && PWPP_FOOT_SKIPPED == PWPP_FOOT_STATUS_SKIPPED &&
                  PWPP_FOOT_OUTSIDE_BLOCKS == PWPP_FOOT_FLAG_OUTSIDE_BLOCKS && PWPP_FOOT_SUB == PWPP_FOOT_TICKS && PWPP_FOOT_MAX_EXTENT == PWPP_FOOT_EXTENT_MAX &&
                  PWPP_FOOT_MAX_STEPS == PWPP_FOOT_STEPS_MAX,
              "the kernels' values");

// What every footprint function checks of the parameters, in the header's order; fills the rule.  Touches no handle.
int footprint_param_args(const pwpp_footprint_params *fp, PwppFootRule &rule) {
    if (fp->front < 0 || fp->front > PWPP_FOOT_MAX_EXTENT) return fail(PWPP_E_ARG, "front %d: 0 .. %d ticks expected", fp->front, PWPP_FOOT_MAX_EXTENT);
    if (fp->rear < 0 || fp->rear > PWPP_FOOT_MAX_EXTENT) return fail(PWPP_E_ARG, "rear %d: 0 .. %d ticks expected", fp->rear, PWPP_FOOT_MAX_EXTENT);
    if (fp->half_width < 0 || fp->half_width > PWPP_FOOT_MAX_EXTENT) return fail(PWPP_E_ARG, "half_width %d: 0 .. %d ticks expected", fp->half_width, PWPP_FOOT_MAX_EXTENT);
    if (fp->flags & ~(int32_t)PWPP_FOOT_OUTSIDE_BLOCKS) return fail(PWPP_E_ARG, "footprint flags %d: 0 or PWPP_FOOT_OUTSIDE_BLOCKS", fp->flags);
    if (fp->pad_[0] != 0 || fp->pad_[1] != 0) return fail(PWPP_E_ARG, "pad_ {%d, %d} of the footprint parameters: 0 expected", fp->pad_[0], fp->pad_[1]);
    rule = PwppFootRule{fp->front, fp->rear, fp->half_width, fp->flags};
    return PWPP_OK;
}
}  // namespace

int pwpp_footprint_grid(pwpp_handle *h, int nx, int ny, int frames, int mem, const int8_t *cost, const int32_t *dist2, const int32_t *reach, const pwpp_reach_params *p,
                        const pwpp_footprint_params *fp, const int32_t *poses, int n_sets, int n_traj, int n_steps, pwpp_footprint_pose_row *pose_rows,
                        pwpp_footprint_traj_row *traj_rows) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!cost || !p || !fp || !poses) return fail(PWPP_E_ARG, "null %s", !cost ? "cost image" : (!p ? "reach parameters" : (!fp ? "footprint parameters" : "poses")));
    size_t n_cells = 0;
    PwppReachRule rule;
    PwppFootRule foot;
    int rc = image_args(nx, ny, frames, kReachWho, n_cells);
    if (rc) return rc;
    if ((rc = reach_param_args(p, nx, ny, dist2 != nullptr, rule, false))) return rc;
    if ((rc = footprint_param_args(fp, foot))) return rc;
    if ((rc = per_frame_count_args(n_sets, frames, "pose sets"))) return rc;
    if (n_traj < 1 || n_traj > PWPP_FOOT_TRAJ_MAX) return fail(PWPP_E_ARG, "%d trajectories: 1 .. %d expected", n_traj, PWPP_FOOT_TRAJ_MAX);
    if (n_steps < 1 || n_steps > PWPP_FOOT_MAX_STEPS) return fail(PWPP_E_ARG, "%d steps: 1 .. %d expected", n_steps, PWPP_FOOT_MAX_STEPS);
    if ((int64_t)frames * (int64_t)n_traj > PWPP_FOOT_POSES_MAX / n_steps)
        return fail(PWPP_E_ARG, "%d frames x %d trajectories x %d steps exceed 2^26", frames, n_traj, n_steps);
    const size_t n_trajs = (size_t)frames * (size_t)n_traj, n_poses = n_trajs * (size_t)n_steps, n_given = (size_t)n_sets * (size_t)n_traj * (size_t)n_steps;
    for (size_t i = 0; i < n_given; ++i)
        if (!pwpp_foot_pose_in_range(poses + 4 * i)) {
            const int32_t *q = poses + 4 * i;
            return fail(PWPP_E_ARG, "pose of set %d, trajectory %d, step %d, {%d, %d, %d, %d}: |px|, |py| <= 2^20 and |ux|, |uy| <= 1024 expected",
                        (int)(i / ((size_t)n_traj * (size_t)n_steps)), (int)(i / (size_t)n_steps % (size_t)n_traj), (int)(i % (size_t)n_steps), q[0], q[1], q[2], q[3]);
        }
    if (!pose_rows && !traj_rows) return fail(PWPP_E_ARG, "null pose rows and null trajectory rows: one of them expected");
    if ((rc = range_args({{cost, n_cells, "cost"}, {dist2, n_cells * 4, "dist2"}, {reach, n_cells * 4, "reach"}, {pose_rows, n_poses * 32, "pose rows"},
                          {traj_rows, n_trajs * 32, "trajectory rows"}}, {}, false)))
        return rc;
    if ((rc = mem_args(mem, "the footprints take"))) return rc;
    if ((rc = alignment_args(mem, {{dist2, 3u, "dist2 image"}, {reach, 3u, "reach image"}, {pose_rows, 3u, "pose rows"}, {traj_rows, 3u, "trajectory rows"}}))) return rc;
    const bool work = traj_rows && !pose_rows && pwpp_footprint_path_of(h->footprint_path, &foot, 0, dist2 != nullptr) == 1;  // (the yardstick's rows, where the caller wants none)
    Staging st(h, h->d_clusters, mem, kClusterAlign);
    const int s_work = st.add(work ? n_poses * 8 : 0, nullptr, Staging::kKept);
    const int s_poses = st.add_upload(std::vector<uint32_t>(reinterpret_cast<const uint32_t *>(poses), reinterpret_cast<const uint32_t *>(poses) + 4 * n_given));
    const int s_cost = st.add_bytes(n_cells, cost, Staging::kIn);
    const int s_dist2 = st.add(dist2 ? n_cells : 0, dist2, Staging::kIn), s_reach = st.add(reach ? n_cells : 0, reach, Staging::kIn);
    const int s_prow = st.add(pose_rows ? n_poses * 8 : 0, pose_rows, Staging::kOut), s_trow = st.add(traj_rows ? n_trajs * 8 : 0, traj_rows, Staging::kOut);
    return run_on_image(h, st, [&] {
        return pwpp_launch_footprints(&rule, &foot, nx, ny, frames, st.dev<const int8_t>(s_cost), dist2 ? st.dev<const int32_t>(s_dist2) : nullptr,
                                      reach ? st.dev<const int32_t>(s_reach) : nullptr, st.dev<const int32_t>(s_poses), n_sets, n_traj, n_steps,
                                      pose_rows ? st.dev<void>(s_prow) : nullptr, traj_rows ? st.dev<void>(s_trow) : nullptr, work ? st.dev<void>(s_work) : nullptr,
                                      h->footprint_path, h->stream);
    });
}

int pwpp_footprint_covers(const pwpp_footprint_params *fp, const int32_t pose[4], int ix, int iy) {
    if (!fp || !pose) return fail(PWPP_E_ARG, "null %s", !fp ? "footprint parameters" : "pose");
    PwppFootRule foot;
    if (const int rc = footprint_param_args(fp, foot)) return rc;
    if (!pwpp_foot_pose_in_range(pose))
        return fail(PWPP_E_ARG, "pose {%d, %d, %d, %d}: |px|, |py| <= 2^20 and |ux|, |uy| <= 1024 expected", pose[0], pose[1], pose[2], pose[3]);
    return pwpp_foot_covers(foot, PwppFootPose{pose[0], pose[1], pose[2], pose[3]}, ix, iy) ? 1 : 0;
}

int pwpp_footprint_pose(const pwpp_ground_grid *g, double x, double y, double yaw, int32_t pose[4]) {
    if (!g || !pose) return fail(PWPP_E_ARG, "null %s", !g ? "grid" : "pose");
    if (const int rc = grid_geometry_args(g)) return rc;
    if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(yaw)) return fail(PWPP_E_ARG, "position (%g, %g), yaw %g: finite values expected", x, y, yaw);
    const double tx = std::floor((x - g->x0) / g->cell * PWPP_FOOT_SUB), ty = std::floor((y - g->y0) / g->cell * PWPP_FOOT_SUB);
    if (!(std::fabs(tx) <= (double)PWPP_FOOT_P_MAX) || !(std::fabs(ty) <= (double)PWPP_FOOT_P_MAX))
        return fail(PWPP_E_ARG, "position (%g, %g) is (%g, %g) ticks from the grid's origin: at most 2^20 expected", x, y, tx, ty);
    pose[0] = (int32_t)tx, pose[1] = (int32_t)ty;
    pose[2] = (int32_t)std::lround(1024.0 * std::cos(yaw)), pose[3] = (int32_t)std::lround(1024.0 * std::sin(yaw));
    return PWPP_OK;
}

// ---- costmap: the occupancy byte, the inflated obstacle distance and the terrain's cost byte folded into one cost byte ----------------
namespace {
static_assert(sizeof(pwpp_costmap_params) == 24, "pwpp_costmap_params is 24 bytes");
static_assert(PWPP_COSTMAP_OCCUPANCY == PWPP_COSTMAP_LAYER_OCCUPANCY && PWPP_COSTMAP_INFLATION == PWPP_COSTMAP_LAYER_INFLATION &&
                  PWPP_COSTMAP_TERRAIN == PWPP_COSTMAP_LAYER_TERRAIN && PWPP_COSTMAP_MAX_CURVE == PWPP_COSTMAP_CURVE_MAX &&
                  (unsigned)PWPP_COSTMAP_WHY_UNKNOWN == PWPP_COSTMAP_WHY_UNKNOWN_BIT && PWPP_OCC_OCCUPIED == 100 && PWPP_OCC_FREE == 0,
              "the kernels' values");
constexpr const char *kCostmapWho = "the costmap takes";

// What every costmap function checks of the parameters and the curve, in the header's order; fills the rule.  Touches no handle.
int costmap_param_args(const pwpp_costmap_params *p, const uint8_t *curve, int n_curve, PwppCostmapRule &rule) {
    const int32_t all = PWPP_COSTMAP_OCCUPANCY | PWPP_COSTMAP_INFLATION | PWPP_COSTMAP_TERRAIN;
    if (p->layers == 0 || (p->layers & ~all)) return fail(PWPP_E_ARG, "layers %d: a mask of 1 (occupancy), 2 (inflation) and 4 (terrain) expected, not 0", p->layers);
    if (p->occupancy_unknown < -1 || p->occupancy_unknown > 100) return fail(PWPP_E_ARG, "occupancy_unknown %d: -1 (stays unknown) .. 100 expected", p->occupancy_unknown);
    if (p->terrain_unknown < -1 || p->terrain_unknown > 100) return fail(PWPP_E_ARG, "terrain_unknown %d: -1 (stays unknown) .. 100 expected", p->terrain_unknown);
    if (p->unknown_below < 1 || p->unknown_below > 101) return fail(PWPP_E_ARG, "unknown_below %d: 1 .. 101 expected (101: unknown always wins)", p->unknown_below);
    if (p->pad_[0] != 0 || p->pad_[1] != 0) return fail(PWPP_E_ARG, "pad_ {%d, %d} of the costmap parameters: 0 expected", p->pad_[0], p->pad_[1]);
    rule = PwppCostmapRule{p->layers, p->occupancy_unknown, p->terrain_unknown, p->unknown_below, 0};
    if (!(p->layers & PWPP_COSTMAP_INFLATION)) return PWPP_OK;
    if (!curve) return fail(PWPP_E_ARG, "null curve with the inflation layer");
    if (n_curve < 1 || n_curve > PWPP_COSTMAP_MAX_CURVE) return fail(PWPP_E_ARG, "n_curve %d: 1 .. 4097 expected", n_curve);
    for (int i = 0; i < n_curve; ++i)
        if (curve[i] > 100) return fail(PWPP_E_ARG, "curve entry %d is %d: 0 .. 100 expected", i, (int)curve[i]);
    rule.n_curve = n_curve;
    return PWPP_OK;
}

// the table as the kernels read it: whole words, the bytes behind n_curve 0 (no words without the inflation layer)
void costmap_curve_words(const PwppCostmapRule &rule, const uint8_t *curve, std::vector<uint32_t> &words) {
    words.assign(((size_t)rule.n_curve + 3) / 4, 0u);
    if (rule.n_curve > 0) std::memcpy(words.data(), curve, (size_t)rule.n_curve);
}

// (the table first; `occ`, `terrain`, `dist2`: the sections of the layers' images -- the caller's, or a stage's)
struct CostmapSections {
    int curve, occ, terrain, dist2, cost, why;
};
CostmapSections costmap_sections(Staging &st, size_t cells, const PwppCostmapRule &rule, const uint8_t *curve, int s_occ, int s_terrain, int s_dist2, int8_t *cost,
                                 uint8_t *why) {
    CostmapSections s;
    std::vector<uint32_t> words;
    costmap_curve_words(rule, curve, words);
    s.curve = rule.n_curve > 0 ? st.add_upload(std::move(words)) : st.add(0, nullptr, Staging::kKept);
    s.occ = s_occ, s.terrain = s_terrain, s.dist2 = s_dist2;
    s.cost = st.add_bytes(cells, cost, Staging::kOut);
    s.why = st.add_bytes(cells, why, Staging::kOut);
    return s;
}
int costmap_launch(pwpp_handle *h, const Staging &st, const CostmapSections &s, const PwppCostmapRule &rule, size_t cells) {
    return pwpp_launch_costmap(&rule, cells, (rule.layers & PWPP_COSTMAP_OCCUPANCY) ? st.dev<const int8_t>(s.occ) : nullptr,
                               (rule.layers & PWPP_COSTMAP_TERRAIN) ? st.dev<const int8_t>(s.terrain) : nullptr,
                               (rule.layers & PWPP_COSTMAP_INFLATION) ? st.dev<const int32_t>(s.dist2) : nullptr,
                               rule.n_curve > 0 ? st.dev<const uint32_t>(s.curve) : nullptr, st.dev<int8_t>(s.cost), st.dev<uint8_t>(s.why), h->costmap_path, h->stream);
}

// The sections of the distances a costmap call computes: the kernels' working image, the count (kept, unless `s_count` names the
// raster's) and dist2 -- the caller's where given, else kept.
DistanceSections costmap_distance_sections(Staging &st, int nx, int ny, int frames, size_t cells, int s_count, int32_t *dist2) {
    DistanceSections s;
    s.work = st.add(pwpp_distance_work_words(nx, ny, frames), nullptr, Staging::kKept);
    s.count = s_count >= 0 ? s_count : st.add(cells, nullptr, Staging::kKept);
    s.dist2 = dist2 ? st.add(cells, dist2, Staging::kOut) : st.add(cells, nullptr, Staging::kKept);
    s.nearest = s.metres = st.add(0, nullptr, Staging::kOut);  // (outputs nobody asks for: null pointers)
    return s;
}
}  // namespace

int pwpp_costmap_grid(pwpp_handle *h, int nx, int ny, int frames, int mem, const int8_t *occupancy, const int8_t *terrain, const int32_t *dist2,
                      const pwpp_costmap_params *p, const uint8_t *curve, int n_curve, int8_t *cost, uint8_t *why) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!p || !cost) return fail(PWPP_E_ARG, "null %s", !p ? "costmap parameters" : "cost image");
    size_t cells = 0;
    int rc = image_args(nx, ny, frames, kCostmapWho, cells);
    if (rc) return rc;
    PwppCostmapRule rule;
    if ((rc = costmap_param_args(p, curve, n_curve, rule))) return rc;
    const bool inflate = (rule.layers & PWPP_COSTMAP_INFLATION) != 0, own_distances = inflate && !dist2;
    if (!occupancy && ((rule.layers & PWPP_COSTMAP_OCCUPANCY) || own_distances))
        return fail(PWPP_E_ARG, "null occupancy image %s", (rule.layers & PWPP_COSTMAP_OCCUPANCY) ? "with the occupancy layer" : "with the inflation layer and no dist2 image");
    if (!terrain && (rule.layers & PWPP_COSTMAP_TERRAIN)) return fail(PWPP_E_ARG, "null terrain image with the terrain layer");
    if ((rc = range_args({{occupancy, cells, "occupancy"}, {terrain, cells, "terrain"}, {dist2, cells * 4, "dist2"}, {cost, cells, "cost"}, {why, cells, "why"}}, {}, false)))
        return rc;
    if ((rc = mem_args(mem, kCostmapWho))) return rc;
    if ((rc = alignment_args(mem, {{dist2, 3u, "dist2 image"}}))) return rc;
    Staging st(h, h->d_clusters, mem, kClusterAlign);
    // (an image whose layer is off is not read: it is not staged either)
    if (!(rule.layers & PWPP_COSTMAP_OCCUPANCY) && !own_distances) occupancy = nullptr;
    if (!(rule.layers & PWPP_COSTMAP_TERRAIN)) terrain = nullptr;
    const int s_occ = st.add_bytes(cells, occupancy, Staging::kIn), s_terrain = st.add_bytes(cells, terrain, Staging::kIn);
    DistanceSections d{};
    if (own_distances) d = costmap_distance_sections(st, nx, ny, frames, cells, -1, nullptr);
    else d.dist2 = st.add(dist2 && inflate ? cells : 0, inflate ? dist2 : nullptr, Staging::kIn);
    const CostmapSections s = costmap_sections(st, cells, rule, curve, s_occ, s_terrain, d.dist2, cost, why);
    return run_on_image(h, st, [&] {
        if (own_distances) {
            int lrc = pwpp_launch_costmap_occupied(cells, st.dev<const int8_t>(s_occ), st.dev<int32_t>(d.count), h->stream);
            if (lrc == 0) lrc = distance_launch(h, st, d, nx, ny, frames, 1, pwpp_costmap_cap(rule.n_curve), 1.0);
            if (lrc != 0) return lrc;
        }
        return costmap_launch(h, st, s, rule, cells);
    });
}

// The stages the enabled layers need -- obstacle raster, visibility, distances, ground raster, the terrain's cost -- and the fold, one enqueued sequence.
int pwpp_costmap_obstacles(pwpp_handle *h, const pwpp_ground_grid *g, float h_min, float h_max, int min_count, const double *origin_xy, int n_origins,
                           int max_range, const pwpp_terrain_params *tp, const pwpp_costmap_params *p, const uint8_t *curve, int n_curve, int frame_first,
                           int frames, int mem, int8_t *cost, uint8_t *why, int8_t *occupancy, int32_t *dist2, int8_t *terrain) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!g || !p || !cost) return fail(PWPP_E_ARG, "null %s", !g ? "grid" : (!p ? "costmap parameters" : "cost image"));
    PwppCostmapRule rule;
    int rc = costmap_param_args(p, curve, n_curve, rule);
    if (rc) return rc;
    const bool with_occ = (rule.layers & PWPP_COSTMAP_OCCUPANCY) != 0, inflate = (rule.layers & PWPP_COSTMAP_INFLATION) != 0,
               with_terrain = (rule.layers & PWPP_COSTMAP_TERRAIN) != 0;
    if (with_occ && !origin_xy) return fail(PWPP_E_ARG, "null origin with the occupancy layer");
    if (with_terrain && !tp) return fail(PWPP_E_ARG, "null terrain parameters with the terrain layer");
    if ((rc = ground_first_args(g, frames, kCostmapWho))) return rc;
    if (with_occ || inflate) {
        if ((rc = obstacle_band_args(g, h_min, h_max)) || (rc = min_count_args(min_count))) return rc;
    }
    std::vector<int32_t> org;
    if (with_occ && (rc = visibility_origin_args(g, h_min, h_max, min_count, origin_xy, n_origins, max_range, frames, org))) return rc;
    // (a layer that is off runs no stage: its image is not written, and its pointer is not looked at)
    if (!with_occ) occupancy = nullptr;
    if (!inflate) dist2 = nullptr;
    if (!with_terrain) terrain = nullptr;
    PwppTerrainRule terrain_rule;
    size_t cells = (size_t)g->nx * (size_t)g->ny * (size_t)frames;  // (as in pwpp_terrain_ground: fits 64 bits; ground_grid_args names one beyond 2^31)
    if (with_terrain && (rc = terrain_args(tp, g->cell, cells, nullptr, nullptr, nullptr, nullptr, nullptr, terrain, terrain_rule))) return rc;
    if ((rc = range_args({{occupancy, cells, "occupancy"}, {terrain, cells, "terrain"}, {dist2, cells * 4, "dist2"}, {cost, cells, "cost"}, {why, cells, "why"}}, {}, false)))
        return rc;
    if ((rc = ground_grid_args(h, g, frame_first, frames, mem, cells))) return rc;
    if ((rc = alignment_args(mem, {{dist2, 3u, "dist2 image"}}))) return rc;
    const int nx = g->nx, ny = g->ny;
    Staging st(h, h->d_clusters, mem, kClusterAlign);
    VisibilitySections v{};
    DistanceSections d{};
    TerrainSections t{};
    v.count = -1;
    if (with_occ) v = visibility_sections(h, st, nx, ny, frames, cells, true, nullptr, org, nullptr, occupancy, true);
    if (inflate) d = costmap_distance_sections(st, nx, ny, frames, cells, v.count, dist2);
    if (with_terrain) t = terrain_cost_sections(st, cells, terrain);
    const CostmapSections s = costmap_sections(st, cells, rule, curve, v.occ, t.cost, d.dist2, cost, why);
    if ((rc = st.begin())) return rc;
    if (with_occ || inflate)
        rc = enqueue_on_obstacles(h, st, g, h_min, h_max, frame_first, frames, inflate ? d.count : v.count, -1, [&](const PwppObstacleScan &) {
            const int lrc = with_occ ? visibility_launch(h, st, v, nx, ny, frames, min_count, org, max_range) : 0;
            return lrc != 0 || !inflate ? lrc : distance_launch(h, st, d, nx, ny, frames, min_count, pwpp_costmap_cap(rule.n_curve), g->cell);
        });
    if (rc == PWPP_OK && with_terrain)
        rc = enqueue_on_ground(h, st, g, frame_first, frames, t.height, -1, [&] { return terrain_launch(h, st, t, terrain_rule, nx, ny, frames); });
    if (rc) return rc;
    const int lrc = costmap_launch(h, st, s, rule, cells);
    return lrc != 0 ? launch_failed(h, lrc) : st.end();
}

// The rule for one cell on the host: pwpp_costmap_fold, the function the kernels call.
int pwpp_costmap_cell(const pwpp_costmap_params *p, const uint8_t *curve, int n_curve, int o, int t, int32_t d, int32_t *cost, uint32_t *why) {
    if (!p) return fail(PWPP_E_ARG, "null costmap parameters");
    PwppCostmapRule rule;
    if (const int rc = costmap_param_args(p, curve, n_curve, rule)) return rc;
    int32_t c;
    uint32_t w;
    pwpp_costmap_fold(rule, curve, (int)(int8_t)o, (int)(int8_t)t, d, c, w);
    if (cost) *cost = c;
    if (why) *why = w;
    return PWPP_OK;
}

// A common inflation table: 100 inside the inscribed radius, then peak * exp(-decay * (distance - inscribed)) down to `radius`.
int pwpp_costmap_curve(double cell, double inscribed, double radius, double decay, int peak, uint8_t *curve, int capacity) {
    if (!curve) return fail(PWPP_E_ARG, "null curve");
    if (!(cell > 0.0) || !std::isfinite(cell)) return fail(PWPP_E_ARG, "cell size %g: finite and positive expected", cell);
    if (!(inscribed >= 0.0) || !(radius >= inscribed) || !std::isfinite(radius))
        return fail(PWPP_E_ARG, "inscribed %g and radius %g: 0 <= inscribed <= radius expected, both finite", inscribed, radius);
    if (!(decay >= 0.0) || !std::isfinite(decay)) return fail(PWPP_E_ARG, "decay %g: finite and at least 0 expected", decay);
    if (peak < 0 || peak > 99) return fail(PWPP_E_ARG, "peak %d: 0 .. 99 expected", peak);
    int n = 1;  // (d = 0 is always inside: 0 <= radius)
    while (n <= PWPP_COSTMAP_MAX_CURVE && std::sqrt((double)n) * cell <= radius) ++n;  // (sqrt(d) * cell rises with d: the first d outside ends the table)
    if (n > PWPP_COSTMAP_MAX_CURVE) return fail(PWPP_E_ARG, "radius %g with cells of %g: the curve would have more than 4097 entries", radius, cell);
    if (capacity < n) return fail(PWPP_E_ARG, "capacity %d: the curve has %d entries", capacity, n);
    for (int d = 0; d < n; ++d) {
        const double r = std::sqrt((double)d) * cell;
        curve[d] = r <= inscribed ? (uint8_t)100 : (uint8_t)(int)std::floor((double)peak * std::exp(-decay * (r - inscribed)));
    }
    return n;
}

// ---- per-beam free space: every return's beam traced from the sensor's cell, the beams that crossed a cell and the lowest of them ----
namespace {
static_assert(PWPP_BEAMS_EYE_MAX == (1 << 30) && PWPP_VIS_MAX_SIDE == 32768, "the limits of the messages");
constexpr const char *kBeamsWho = "the beams take";

// what both entry points check of max_range, min_pass and the clearance in units
int beam_param_args(int max_range, int min_pass, int64_t clearance) {
    if (max_range < 0 || max_range > PWPP_VIS_MAX_SIDE) return fail(PWPP_E_ARG, "max_range %d: 0 (unlimited) .. 32768 cells expected", max_range);
    if (min_pass < 1) return fail(PWPP_E_ARG, "min_pass %d: at least 1 expected", min_pass);
    if (clearance < 0) return fail(PWPP_E_ARG, "clearance %lld: at least 0 expected", (long long)clearance);
    return PWPP_OK;
}

// ... and of the caller's arrays among each other: occupancy may be occupancy_in itself, nothing else may meet
int beam_range_args(size_t cells, const int32_t *hits, const int32_t *zmin, const int32_t *target, const int8_t *occupancy_in, const int32_t *passes,
                    const int32_t *low, const int8_t *occupancy) {
    return range_args({{hits, cells * 4, "hits"}, {zmin, cells * 4, "zmin"}, {target, cells * 4, "target"}, {occupancy_in, cells, "occupancy_in"},
                       {occupancy, cells, "occupancy"}, {passes, cells * 4, "passes"}, {low, cells * 4, "low"}},
                      {{3, 4}}, false);
}

// (the origins first; `org`: n_origins x {ox, oy, eye}, checked.  One origin travels as arguments.)
struct BeamSections {
    int org, hits, zmin, target, occ_in, passes, low, occ;
};
void beam_out_sections(Staging &st, size_t cells, const int8_t *occupancy_in, int32_t *passes, int32_t *low, int8_t *occupancy, BeamSections &s) {
    s.occ_in = st.add_bytes(cells, occupancy_in, Staging::kIn);
    s.passes = st.add(cells, passes, Staging::kOut), s.low = st.add(cells, low, Staging::kOut);
    s.occ = st.add_bytes(cells, occupancy, Staging::kOut);
}
int beam_launch(pwpp_handle *h, const Staging &st, const BeamSections &s, int nx, int ny, int frames, const std::vector<int32_t> &org, int max_range, int min_pass,
                int clearance) {
    return pwpp_launch_beam_grid(nx, ny, frames, st.dev<const int32_t>(s.hits), st.dev<const int32_t>(s.zmin), st.dev<const int32_t>(s.target),
                                 st.dev<const int8_t>(s.occ_in), org[0], org[1], org[2], org.size() > 3 ? st.dev<const int32_t>(s.org) : nullptr, max_range, min_pass,
                                 clearance, h->beams_path, st.dev<int32_t>(s.passes), st.dev<int32_t>(s.low), st.dev<int8_t>(s.occ), h->stream);
}

// The longest selection of a frame range of the last call: the ground list (which & 1), the non-ground list (which & 2) or both
int longest_beam_list(const pwpp_handle *h, int which, int frame_first, int frames) {
    int64_t longest = 0;
    for (int f = frame_first; f < frame_first + frames; ++f) {
        const auto &r = h->h_results.p[f];
        longest = std::max(longest, ((which & 1) ? (int64_t)std::max(r.n_ground, 0) : 0) + ((which & 2) ? (int64_t)std::max(r.n_nonground, 0) : 0));
    }
    return (int)std::min<int64_t>(longest, INT32_MAX);
}
int beam_which_args(const pwpp_ground_grid *g, int which) {
    if (g->flags != 0) return fail(PWPP_E_ARG, "grid flags %d: 0 expected by the beams' endpoints", g->flags);
    if (which < 1 || which > 3) return fail(PWPP_E_ARG, "which %d: 1 (ground), 2 (non-ground) or 3 (both) expected", which);
    return PWPP_OK;
}
}  // namespace

// The rule for one crossed cell on the host: pwpp_beams_height, the function the kernels call.
int32_t pwpp_beam_height(int32_t eye, int32_t z, int k, int n) {
    if (n < 2 || k < 1 || k >= n || n > PWPP_VIS_MAX_SIDE || eye < -PWPP_BEAMS_EYE_MAX || eye > PWPP_BEAMS_EYE_MAX || z == PWPP_VIEW_NO_HEIGHT) {
        fail(PWPP_E_ARG, "beam height at k %d of n %d, eye %d: 1 <= k < n <= 32768, |eye| <= 2^30 and a height expected", k, n, eye);
        return PWPP_VIEW_NO_HEIGHT;
    }
    return pwpp_beams_height(eye, z, (uint32_t)k, (uint32_t)n);
}

// The selected index lists of the last call per cell of the grid: hits, then zmin.
int pwpp_rasterize_beams(pwpp_handle *h, const pwpp_ground_grid *g, int which, int frame_first, int frames, int mem, int32_t *hits, int32_t *zmin) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!g || !hits || !zmin) return fail(PWPP_E_ARG, "null %s", !g ? "grid" : (!hits ? "hits image" : "zmin image"));
    int rc = beam_which_args(g, which);
    if (rc) return rc;
    size_t cells = 0;
    if ((rc = ground_grid_args(h, g, frame_first, frames, mem, cells))) return rc;
    if ((rc = range_args({{hits, cells * 4, "hits"}, {zmin, cells * 4, "zmin"}}, {}, false))) return rc;
    Staging st(h, h->d_ground_stage, mem);
    const int s_hits = st.add(cells, hits, Staging::kOut), s_zmin = st.add(cells, zmin, Staging::kOut);
    if ((rc = st.begin())) return rc;
    PwppObstacleScan scan;
    if ((rc = obstacle_scan(h, g, 0.0f, 0.0f, frame_first, frames, scan))) return rc;
    const int lrc = pwpp_launch_beam_ends(&scan, which, longest_beam_list(h, which, frame_first, frames), st.dev<int32_t>(s_hits), st.dev<int32_t>(s_zmin), h->stream);
    return lrc != 0 ? launch_failed(h, lrc) : st.end();
}

int pwpp_beam_grid(pwpp_handle *h, int nx, int ny, int frames, int mem, const int32_t *hits, const int32_t *zmin, const int32_t *target,
                   const int8_t *occupancy_in, const int32_t *origin, int n_origins, int max_range, int min_pass, int clearance, int32_t *passes, int32_t *low,
                   int8_t *occupancy) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!hits || !zmin || !origin || !passes || !low)
        return fail(PWPP_E_ARG, "null %s", !hits ? "hits image" : (!zmin ? "zmin image" : (!origin ? "origin" : (!passes ? "passes image" : "low image"))));
    size_t cells = 0;
    int rc = image_args(nx, ny, frames, kBeamsWho, cells);
    if (rc) return rc;
    if ((rc = beam_param_args(max_range, min_pass, clearance))) return rc;
    if ((rc = per_frame_count_args(n_origins, frames, "origins"))) return rc;
    if ((rc = cells_inside_args(origin, n_origins, nx, ny, "origin", 3))) return rc;
    for (int i = 0; i < n_origins; ++i)
        if (origin[3 * i + 2] < -PWPP_BEAMS_EYE_MAX || origin[3 * i + 2] > PWPP_BEAMS_EYE_MAX)
            return fail(PWPP_E_ARG, "origin %d: its eye %d lies outside +-2^30", i, origin[3 * i + 2]);
    if ((rc = beam_range_args(cells, hits, zmin, target, occupancy_in, passes, low, occupancy))) return rc;
    if ((rc = mem_args(mem, kBeamsWho))) return rc;
    if ((rc = alignment_args(mem, {{hits, 3u, "hits image"}, {zmin, 3u, "zmin image"}, {target, 3u, "target image"}, {passes, 3u, "passes image"}, {low, 3u, "low image"}})))
        return rc;
    const std::vector<int32_t> org(origin, origin + 3 * (size_t)n_origins);
    Staging st(h, h->d_clusters, mem, kClusterAlign);
    BeamSections s;
    s.org = frame_cells_section(st, org, 3);
    s.hits = st.add(cells, hits, Staging::kIn), s.zmin = st.add(cells, zmin, Staging::kIn), s.target = add_image(st, cells, target, false);
    beam_out_sections(st, cells, occupancy_in, passes, low, occupancy, s);
    return run_on_image(h, st, [&] { return beam_launch(h, st, s, nx, ny, frames, org, max_range, min_pass, clearance); });
}

// The endpoints' raster, the ground raster, the quantiser and the beams, one enqueued sequence.
int pwpp_beam_ground(pwpp_handle *h, const pwpp_ground_grid *g, int which, const double *origin_xyz, int n_origins, int max_range, int min_pass, double clearance,
                     int frame_first, int frames, int mem, const int8_t *occupancy_in, int32_t *passes, int32_t *low, int8_t *occupancy, int32_t *hits,
                     int32_t *zmin) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!g || !origin_xyz || !passes || !low) return fail(PWPP_E_ARG, "null %s", !g ? "grid" : (!origin_xyz ? "origin" : (!passes ? "passes image" : "low image")));
    if (g->flags & ~(int32_t)PWPP_GRID_GROUND_ONLY) return fail(PWPP_E_ARG, "grid flags %d: 0 or PWPP_GRID_GROUND_ONLY", g->flags);
    if (which < 1 || which > 3) return fail(PWPP_E_ARG, "which %d: 1 (ground), 2 (non-ground) or 3 (both) expected", which);
    int rc = grid_geometry_args(g);  // (the origins need the grid)
    if (rc || (rc = side_args(g->nx, g->ny, kBeamsWho))) return rc;
    if (!(clearance >= 0.0) || !std::isfinite(clearance)) return fail(PWPP_E_ARG, "clearance %g m: finite and at least 0 expected", clearance);
    const int32_t clear_units = pwpp_view_units(clearance);
    if ((rc = beam_param_args(max_range, min_pass, clear_units))) return rc;
    if ((rc = per_frame_count_args(n_origins, frames, "origins"))) return rc;
    std::vector<int32_t> org;
    if ((rc = frame_cells_of(g, origin_xyz, n_origins, "origin", org, 3))) return rc;  // (an eye is a quantised height: within +-2^30)
    size_t cells = (size_t)g->nx * (size_t)g->ny * (size_t)(frames > 0 ? frames : 0);  // (the byte ranges of the overlap check; ground_grid_args names one beyond 2^31)
    if ((rc = beam_range_args(cells, hits, zmin, nullptr, occupancy_in, passes, low, occupancy))) return rc;
    if ((rc = ground_grid_args(h, g, frame_first, frames, mem, cells))) return rc;
    if ((rc = alignment_args(mem, {{hits, 3u, "hits image"}, {zmin, 3u, "zmin image"}, {passes, 3u, "passes image"}, {low, 3u, "low image"}}))) return rc;
    const int nx = g->nx, ny = g->ny;
    Staging st(h, h->d_clusters, mem, kClusterAlign);
    BeamSections s;
    s.org = frame_cells_section(st, org, 3);
    s.hits = add_image(st, cells, hits, true), s.zmin = add_image(st, cells, zmin, true);
    const int s_ground = st.add(cells, nullptr, Staging::kKept);
    s.target = st.add(cells, nullptr, Staging::kKept);
    beam_out_sections(st, cells, occupancy_in, passes, low, occupancy, s);
    if ((rc = st.begin())) return rc;
    PwppObstacleScan scan;
    pwpp_ground_grid ends = *g;
    ends.flags = 0;  // (the endpoints' raster reads no flags)
    if ((rc = obstacle_scan(h, &ends, 0.0f, 0.0f, frame_first, frames, scan))) return rc;
    int lrc = pwpp_launch_beam_ends(&scan, which, longest_beam_list(h, which, frame_first, frames), st.dev<int32_t>(s.hits), st.dev<int32_t>(s.zmin), h->stream);
    if (lrc != 0) return launch_failed(h, lrc);
    rc = enqueue_on_ground(h, st, g, frame_first, frames, s_ground, -1, [&] {
        lrc = pwpp_launch_viewshed_quantise(cells, st.dev<const float>(s_ground), nullptr, st.dev<int32_t>(s.target), nullptr, h->stream);
        return lrc != 0 ? lrc : beam_launch(h, st, s, nx, ny, frames, org, max_range, min_pass, clear_units);
    });
    return rc ? rc : st.end();
}

// ---- cluster tracks: the rows of a current label image against those of the previous one, and ids that persist ------------------------
namespace {
static_assert(sizeof(pwpp_cluster_link) == 16 && sizeof(PwppClusterLink) == 16 && alignof(pwpp_cluster_link) == 4, "pwpp_cluster_link is 16 bytes of 4-byte fields");
static_assert(offsetof(pwpp_cluster_link, other) == offsetof(PwppClusterLink, other) && offsetof(pwpp_cluster_link, overlap) == offsetof(PwppClusterLink, overlap) &&
                  offsetof(pwpp_cluster_link, cells) == offsetof(PwppClusterLink, cells) && offsetof(pwpp_cluster_link, links) == offsetof(PwppClusterLink, links),
              "the kernels' row of a link table");
constexpr const char *kTracksWho = "the association takes";

// The caller's arrays of an association besides the two images: what both entry points pass on.
struct TrackArrays {
    const double *pose;
    int n_poses;
    pwpp_cluster_link *curr_links, *prev_links;
    int32_t *n_pairs;
    const int32_t *id_prev, *next_id;
    int32_t *id_curr, *next_id_out;
};

// What both entry points check from the gate on, in the header's order, after the images' and grids' own checks (frames >= 1): the
// parameters, the count of poses, the id set, the overlaps among the caller's arrays (`curr` is an output of pwpp_track_obstacles).
// Fills the rule.  Touches no handle.
int tracks_args(int frames, size_t cells_c, size_t cells_p, const int32_t *curr, const int32_t *prev, const TrackArrays &t, int gate, int min_overlap, int max_rows,
                int max_pairs, PwppTracksRule &rule) {
    if (gate < 0 || gate > PWPP_TRACKS_MAX_GATE) return fail(PWPP_E_ARG, "gate %d: 0 .. 4 expected", gate);
    if (min_overlap < 1) return fail(PWPP_E_ARG, "min_overlap %d: at least 1 expected", min_overlap);
    if (max_rows < 1) return fail(PWPP_E_ARG, "max_rows %d: at least 1 expected", max_rows);
    if ((int64_t)frames * max_rows > PWPP_TRACKS_MAX_TOTAL) return fail(PWPP_E_ARG, "%d frames x max_rows %d exceed 2^24", frames, max_rows);
    if (max_pairs < 1) return fail(PWPP_E_ARG, "max_pairs %d: at least 1 expected", max_pairs);
    if ((int64_t)frames * max_pairs > PWPP_TRACKS_MAX_TOTAL) return fail(PWPP_E_ARG, "%d frames x max_pairs %d exceed 2^24", frames, max_pairs);
    if (const int rc = per_frame_count_args(t.n_poses, frames, "poses")) return rc;
    const int given = (t.id_prev != nullptr) + (t.next_id != nullptr) + (t.id_curr != nullptr) + (t.next_id_out != nullptr);
    if (given != 0 && given != 4)
        return fail(PWPP_E_ARG, "null %s with other id arrays given: id_prev, next_id, id_curr and next_id_out all or none expected",
                    !t.id_prev ? "id_prev" : (!t.next_id ? "next_id" : (!t.id_curr ? "id_curr" : "next_id_out")));
    const size_t rows = (size_t)frames * (size_t)max_rows;
    if (const int rc = range_args({{curr, cells_c * 4, "curr"}, {prev, cells_p * 4, "prev"}, {t.curr_links, rows * 16, "curr_links"}, {t.prev_links, rows * 16, "prev_links"},
                                   {t.n_pairs, (size_t)frames * 4, "n_pairs"}, {t.id_prev, rows * 4, "id_prev"}, {t.next_id, (size_t)frames * 4, "next_id"},
                                   {t.id_curr, rows * 4, "id_curr"}, {t.next_id_out, (size_t)frames * 4, "next_id_out"}},
                                  {}, false))
        return rc;
    rule = PwppTracksRule{gate, min_overlap, max_rows, max_pairs, pwpp_tracks_slots(max_pairs), given == 4 ? 1 : 0};
    return PWPP_OK;
}

// (after mem: every array of the association 4-byte aligned in PWPP_MEM_DEVICE)
int tracks_alignment_args(int mem, const int32_t *curr, const int32_t *prev, const TrackArrays &t) {
    return alignment_args(mem, {{curr, 3u, "curr image"}, {prev, 3u, "prev image"}, {t.curr_links, 3u, "curr_links"}, {t.prev_links, 3u, "prev_links"},
                                {t.n_pairs, 3u, "n_pairs"}, {t.id_prev, 3u, "id_prev"}, {t.next_id, 3u, "next_id"}, {t.id_curr, 3u, "id_curr"},
                                {t.next_id_out, 3u, "next_id_out"}});
}

// the geometry of the vote: the current grid in the role of the fusion's map, the previous one in the role of its frame images
PwppFusionGeometry tracks_geometry(const pwpp_ground_grid *gc, const pwpp_ground_grid *gp) {
    PwppFusionGeometry G{gc->x0, gc->y0, gc->cell, gp->x0, gp->y0, gp->cell, gc->nx, gc->ny, gp->nx, gp->ny, 0.0};
    pwpp_fuse_reciprocal(gp->cell, G.inv_cell);
    return G;
}

// (the kernels' working words and the uploaded poses first; `s_curr` is the current image's section: the caller's, or the labelling's)
struct TrackSections {
    int work, pose, curr, prev, curr_links, prev_links, n_pairs, id_prev, next_id, id_curr, next_id_out;
};
TrackSections track_sections(Staging &st, int frames, size_t cells_p, int s_curr, const int32_t *prev, const TrackArrays &t, const PwppTracksRule &rule) {
    TrackSections s;
    const size_t rows = (size_t)frames * (size_t)rule.max_rows, ids = rule.with_ids ? rows : 0, nexts = rule.with_ids ? (size_t)frames : 0;
    s.work = st.add(pwpp_tracks_work_words(frames, rule.max_rows, rule.max_pairs), nullptr, Staging::kKept);
    std::vector<uint32_t> words((size_t)t.n_poses * 12);
    std::memcpy(words.data(), t.pose, (size_t)t.n_poses * 6 * sizeof(double));
    s.pose = st.add_upload(std::move(words));
    s.curr = s_curr;
    s.prev = st.add(cells_p, prev, Staging::kIn);
    s.curr_links = st.add(rows * 4, t.curr_links, Staging::kOut), s.prev_links = st.add(rows * 4, t.prev_links, Staging::kOut);
    s.n_pairs = st.add(t.n_pairs ? (size_t)frames : 0, t.n_pairs, Staging::kOut);
    s.id_prev = st.add(ids, t.id_prev, Staging::kIn), s.next_id = st.add(nexts, t.next_id, Staging::kIn);
    s.id_curr = st.add(ids, t.id_curr, Staging::kOut), s.next_id_out = st.add(nexts, t.next_id_out, Staging::kOut);
    return s;
}
int track_launch(pwpp_handle *h, const Staging &st, const TrackSections &s, const PwppFusionGeometry &G, const PwppTracksRule &rule, int frames, int n_poses,
                 bool with_n_pairs) {
    return pwpp_launch_tracks(&G, &rule, frames, st.dev<const int32_t>(s.curr), st.dev<const int32_t>(s.prev), st.dev<const double>(s.pose), n_poses,
                              st.dev<void>(s.curr_links), st.dev<void>(s.prev_links), with_n_pairs ? st.dev<int32_t>(s.n_pairs) : nullptr,
                              rule.with_ids ? st.dev<const int32_t>(s.id_prev) : nullptr, rule.with_ids ? st.dev<const int32_t>(s.next_id) : nullptr,
                              rule.with_ids ? st.dev<int32_t>(s.id_curr) : nullptr, rule.with_ids ? st.dev<int32_t>(s.next_id_out) : nullptr,
                              st.dev<uint32_t>(s.work), h->stream);
}
}  // namespace

int pwpp_associate_grid(pwpp_handle *h, const pwpp_ground_grid *gc, const pwpp_ground_grid *gp, int frames, int mem, const int32_t *curr, const int32_t *prev,
                        const double *pose, int n_poses, int gate, int min_overlap, int max_rows, int max_pairs, pwpp_cluster_link *curr_links,
                        pwpp_cluster_link *prev_links, int32_t *n_pairs, const int32_t *id_prev, const int32_t *next_id, int32_t *id_curr, int32_t *next_id_out) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!gc || !gp || !curr || !prev || !pose || !curr_links || !prev_links)
        return fail(PWPP_E_ARG, "null %s",
                    !gc ? "current grid" : (!gp ? "previous grid" : (!curr ? "current image" : (!prev ? "previous image" : (!pose ? "pose" : (!curr_links ? "curr_links" : "prev_links"))))));
    size_t cells_c = 0, cells_p = 0;
    int rc = image_args(gc->nx, gc->ny, frames, kTracksWho, cells_c);
    if (rc || (rc = image_args(gp->nx, gp->ny, frames, kTracksWho, cells_p))) return rc;
    if (gc->flags != 0 || gp->flags != 0)
        return fail(PWPP_E_ARG, "grid flags %d of the %s grid: the association takes 0", gc->flags != 0 ? gc->flags : gp->flags, gc->flags != 0 ? "current" : "previous");
    if ((rc = grid_geometry_args(gc)) || (rc = grid_geometry_args(gp))) return rc;
    const TrackArrays t{pose, n_poses, curr_links, prev_links, n_pairs, id_prev, next_id, id_curr, next_id_out};
    PwppTracksRule rule;
    if ((rc = tracks_args(frames, cells_c, cells_p, curr, prev, t, gate, min_overlap, max_rows, max_pairs, rule))) return rc;
    if ((rc = mem_args(mem, kTracksWho))) return rc;
    if ((rc = tracks_alignment_args(mem, curr, prev, t))) return rc;
    const PwppFusionGeometry G = tracks_geometry(gc, gp);
    Staging st(h, h->d_clusters, mem, kClusterAlign);
    const int s_curr = st.add(cells_c, curr, Staging::kIn);
    const TrackSections s = track_sections(st, frames, cells_p, s_curr, prev, t, rule);
    return run_on_image(h, st, [&] { return track_launch(h, st, s, G, rule, frames, n_poses, n_pairs != nullptr); });
}

// pwpp_label_obstacles as it stands, its label image kept where it lies (the caller's, or the cluster buffer's in PWPP_MEM_HOST), and
// pwpp_associate_grid of it against the caller's previous image on the same grid, one enqueued sequence.
int pwpp_track_obstacles(pwpp_handle *h, const pwpp_ground_grid *g, float h_min, float h_max, int min_count, int connectivity, int frame_first, int frames, int mem,
                         int32_t *label, int32_t *count, float *top, pwpp_obstacle_cluster *clusters, int32_t *n_clusters, int max_clusters, int32_t *point_cluster,
                         const int32_t *prev_label, const double *pose, int n_poses, int gate, int min_overlap, int max_pairs, pwpp_cluster_link *curr_links,
                         pwpp_cluster_link *prev_links, int32_t *n_pairs, const int32_t *id_prev, const int32_t *next_id, int32_t *id_curr, int32_t *next_id_out) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!g || !label || !prev_label || !pose || !curr_links || !prev_links)
        return fail(PWPP_E_ARG, "null %s",
                    !g ? "grid" : (!label ? "label image" : (!prev_label ? "previous label image" : (!pose ? "pose" : (!curr_links ? "curr_links" : "prev_links")))));
    const LabelArrays a{label, count, top, clusters, n_clusters, max_clusters, point_cluster};
    size_t cells = 0;
    int rc = label_first_args(h, g, h_min, h_max, min_count, connectivity, frame_first, frames, mem, a, kTracksWho, cells);
    if (rc) return rc;
    if (g->flags != 0) return fail(PWPP_E_ARG, "grid flags %d of the current grid: the association takes 0", g->flags);
    const TrackArrays t{pose, n_poses, curr_links, prev_links, n_pairs, id_prev, next_id, id_curr, next_id_out};
    PwppTracksRule rule;
    if ((rc = tracks_args(frames, cells, cells, label, prev_label, t, gate, min_overlap, max_clusters, max_pairs, rule))) return rc;
    if ((rc = tracks_alignment_args(mem, label, prev_label, t))) return rc;
    const PwppFusionGeometry G = tracks_geometry(g, g);
    return run_on_labels(h, g, h_min, h_max, min_count, connectivity, frame_first, frames, mem, cells, a, [&](Staging &st, int s_label) {
        const TrackSections ts = track_sections(st, frames, cells, s_label, prev_label, t, rule);
        return [&, ts] { return track_launch(h, st, ts, G, rule, frames, n_poses, n_pairs != nullptr); };
    });
}

// ---- map evidence: what the fused map holds under the cells of every cluster row of a label image -------------------------------------
namespace {
static_assert(sizeof(pwpp_cluster_evidence) == 32 && sizeof(PwppClusterEvidence) == 32 && alignof(pwpp_cluster_evidence) == 8, "pwpp_cluster_evidence is 32 bytes, 8-byte aligned");
static_assert(offsetof(pwpp_cluster_evidence, sum) == offsetof(PwppClusterEvidence, sum) && offsetof(pwpp_cluster_evidence, cells) == offsetof(PwppClusterEvidence, cells) &&
                  offsetof(pwpp_cluster_evidence, landed) == offsetof(PwppClusterEvidence, landed) && offsetof(pwpp_cluster_evidence, occupied) == offsetof(PwppClusterEvidence, occupied) &&
                  offsetof(pwpp_cluster_evidence, free) == offsetof(PwppClusterEvidence, free) && offsetof(pwpp_cluster_evidence, unknown) == offsetof(PwppClusterEvidence, unknown) &&
                  offsetof(pwpp_cluster_evidence, verdict) == offsetof(PwppClusterEvidence, verdict),
              "the kernels' row of the evidence");
static_assert(sizeof(pwpp_evidence_rule) == sizeof(PwppEvidenceRule), "the kernels' rule");
static_assert(PWPP_EVID_NONE == PWPP_EV_NONE && PWPP_EVID_UNDECIDED == PWPP_EV_UNDECIDED && PWPP_EVID_STATIC == PWPP_EV_STATIC && PWPP_EVID_MOVING == PWPP_EV_MOVING &&
                  PWPP_EVID_CELL_NONE == PWPP_EV_CELL_NONE && PWPP_EVID_LDS_ROWS == PWPP_EV_LDS_ROWS,
              "the kernels' verdicts, class byte and LDS rows");
constexpr const char *kEvidenceWho = "the map evidence takes";

// The caller's arrays of an evidence call besides the label image: what both entry points pass on.
struct EvidenceArrays {
    const int8_t *occ_in;
    const double *pose;
    int n_poses;
    const int32_t *map_of_frame;
    const int16_t *map;
    pwpp_cluster_evidence *rows;
    int8_t *cell_class, *occ_out;
};

// What a checked call hands to the kernels besides its arrays: geometry, rule, thresholds and the words to upload -- the poses
// first (8-byte aligned at the section's start), then every frame's map, the rule of map_of_frame resolved.
struct EvidencePlan {
    PwppMatchGeometry G;
    PwppEvidenceRule R;
    int32_t occupied_at = 0, free_at = 0;
    int n_poses = 0, max_rows = 0;
    size_t map_cells = 0;  // NX * NY * n_maps
    std::vector<uint32_t> words;
    size_t at_maps() const { return (size_t)n_poses * 12; }
};

// the rule's ranges, named: one text with the kernels' launcher (pwpp_evid_rule_check)
int evidence_rule_args(const pwpp_evidence_rule *rule, PwppEvidenceRule &R) {
    R = PwppEvidenceRule{rule->gate, rule->min_cells, rule->moving_share, rule->static_share};
    switch (pwpp_evid_rule_check(R)) {
        case 1: return fail(PWPP_E_ARG, "gate %d: 0 .. 4 expected", R.gate);
        case 2: return fail(PWPP_E_ARG, "min_cells %d: at least 1 expected", R.min_cells);
        case 3: return fail(PWPP_E_ARG, "moving_share %d: 1 .. 256 expected", R.moving_share);
        case 4: return fail(PWPP_E_ARG, "static_share %d: 1 .. 256 expected", R.static_share);
        default: return PWPP_OK;
    }
}

// What both entry points check from the map's origin on, in the header's order, after the sizes of the images and the map, the
// grid's flags and its own geometry (frames >= 1; `label` is an output of pwpp_evidence_obstacles).  Fills the plan.  Touches no handle.
int evidence_args(const pwpp_ground_grid *g, int frames, size_t cells, const int32_t *label, const EvidenceArrays &a, const pwpp_fusion_map *m, int n_maps,
                  const pwpp_evidence_rule *rule, int max_rows, EvidencePlan &plan) {
    if (!(m->cell > 0.0) || !std::isfinite(m->cell) || !std::isfinite(m->x0) || !std::isfinite(m->y0))
        return fail(PWPP_E_ARG, "map origin and cell size must be finite, the cell size positive");
    if (m->free_at < -32768 || m->free_at >= m->occupied_at || m->occupied_at > 32767)
        return fail(PWPP_E_ARG, "thresholds free_at %d, occupied_at %d: -32768 <= free_at < occupied_at <= 32767 expected", m->free_at, m->occupied_at);
    if (const int rc = evidence_rule_args(rule, plan.R)) return rc;
    if (max_rows < 1) return fail(PWPP_E_ARG, "max_rows %d: at least 1 expected", max_rows);
    if ((int64_t)frames * max_rows > PWPP_EV_MAX_TOTAL) return fail(PWPP_E_ARG, "%d frames x max_rows %d exceed 2^24", frames, max_rows);
    if (const int rc = per_frame_count_args(a.n_poses, frames, "poses")) return rc;
    const FrameMaps map_of{a.map_of_frame, n_maps};
    if (const int rc = map_of.args(frames)) return rc;
    if ((a.occ_in != nullptr) != (a.occ_out != nullptr))
        return fail(PWPP_E_ARG, "null %s with %s given: both or neither expected", a.occ_in ? "occupancy_out" : "occupancy_in", a.occ_in ? "occupancy_in" : "occupancy_out");
    if (const int rc = range_args({{label, cells * 4, "label"}, {a.occ_in, cells, "occupancy_in"}, {a.map, plan.map_cells * sizeof(int16_t), "map"},
                                   {a.rows, (size_t)frames * (size_t)max_rows * sizeof(pwpp_cluster_evidence), "rows"}, {a.cell_class, cells, "cell_class"},
                                   {a.occ_out, cells, "occupancy_out"}},
                                  {{1, 5}}, false))
        return rc;
    plan.G = PwppMatchGeometry{m->x0, m->y0, m->cell, g->x0, g->y0, g->cell, m->nx, m->ny, g->nx, g->ny, 0.0};
    pwpp_fuse_reciprocal(m->cell, plan.G.inv_CELL);
    plan.occupied_at = m->occupied_at, plan.free_at = m->free_at, plan.n_poses = a.n_poses, plan.max_rows = max_rows;
    try {
        plan.words.assign(plan.at_maps() + (size_t)frames, 0u);
    } catch (const std::bad_alloc &) {
        return fail(PWPP_E_NOMEM, "no host memory for %d poses and %d frames", a.n_poses, frames);
    }
    std::memcpy(plan.words.data(), a.pose, (size_t)a.n_poses * 6 * sizeof(double));
    for (int i = 0; i < frames; ++i) plan.words[plan.at_maps() + (size_t)i] = (uint32_t)map_of(i);
    return PWPP_OK;
}

// (after mem: what PWPP_MEM_DEVICE asks of the arrays; the byte images are byte aligned, no more)
int evidence_alignment_args(int mem, const int32_t *label, const EvidenceArrays &a) {
    return alignment_args(mem, {{a.rows, 7u, "rows"}, {label, 3u, "label image"}, {a.map, 1u, "map"}});
}

// (the plan's words first: they move into the staging; `s_label` is the label image's section: the caller's, or the labelling's)
struct EvidenceSections {
    int up, label, occ_in, map, rows, cell_class, occ_out;
};
EvidenceSections evidence_sections(Staging &st, EvidencePlan &plan, int frames, size_t cells, int s_label, const EvidenceArrays &a) {
    EvidenceSections s;
    s.up = st.add_upload(std::move(plan.words));
    s.label = s_label;
    s.occ_in = st.add_bytes(cells, a.occ_in, Staging::kIn);
    s.map = st.add((plan.map_cells + 1) / 2, a.map, Staging::kIn, plan.map_cells * sizeof(int16_t));
    s.rows = st.add((size_t)frames * (size_t)plan.max_rows * (sizeof(pwpp_cluster_evidence) / 4), a.rows, Staging::kOut);
    s.cell_class = st.add_bytes(cells, a.cell_class, Staging::kOut);
    s.occ_out = st.add_bytes(cells, a.occ_out, Staging::kOut);
    return s;
}
int evidence_launch(pwpp_handle *h, const Staging &st, const EvidenceSections &s, const EvidencePlan &plan, int frames, const EvidenceArrays &a) {
    return pwpp_launch_evidence(&plan.G, &plan.R, plan.occupied_at, plan.free_at, frames, st.dev<const int32_t>(s.label), a.occ_in ? st.dev<const int8_t>(s.occ_in) : nullptr,
                                st.dev<const double>(s.up), plan.n_poses, st.dev<const int32_t>(s.up) + plan.at_maps(), st.dev<const int16_t>(s.map), plan.max_rows,
                                st.dev<void>(s.rows), a.cell_class ? st.dev<int8_t>(s.cell_class) : nullptr, a.occ_out ? st.dev<int8_t>(s.occ_out) : nullptr,
                                h->evidence_path, h->stream);
}
}  // namespace

int pwpp_evidence_grid(pwpp_handle *h, const pwpp_ground_grid *g, int frames, int mem, const int32_t *label, const int8_t *occupancy_in, const double *pose, int n_poses,
                       const int32_t *map_of_frame, const pwpp_fusion_map *m, int n_maps, const int16_t *map, const pwpp_evidence_rule *rule, int max_rows,
                       pwpp_cluster_evidence *rows, int8_t *cell_class, int8_t *occupancy_out) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!g || !label || !pose || !m || !map || !rule || !rows)
        return fail(PWPP_E_ARG, "null %s",
                    !g ? "grid" : (!label ? "label image" : (!pose ? "pose" : (!m ? "map description" : (!map ? "map" : (!rule ? "rule" : "rows"))))));
    size_t cells = 0;
    EvidencePlan plan;
    int rc = image_args(g->nx, g->ny, frames, kEvidenceWho, cells);
    if (rc || (rc = image_args(m->nx, m->ny, n_maps, kEvidenceWho, plan.map_cells))) return rc;
    if (g->flags != 0) return fail(PWPP_E_ARG, "grid flags %d: the map evidence's frame grid takes 0", g->flags);
    if ((rc = grid_geometry_args(g))) return rc;
    const EvidenceArrays a{occupancy_in, pose, n_poses, map_of_frame, map, rows, cell_class, occupancy_out};
    if ((rc = evidence_args(g, frames, cells, label, a, m, n_maps, rule, max_rows, plan))) return rc;
    if ((rc = mem_args(mem, kEvidenceWho))) return rc;
    if ((rc = evidence_alignment_args(mem, label, a))) return rc;
    Staging st(h, h->d_clusters, mem, kClusterAlign);
    const int s_label = st.add(cells, label, Staging::kIn);
    const EvidenceSections s = evidence_sections(st, plan, frames, cells, s_label, a);
    return run_on_image(h, st, [&] { return evidence_launch(h, st, s, plan, frames, a); });
}

// pwpp_label_obstacles as it stands, its label image kept where it lies, and pwpp_evidence_grid of it, one enqueued sequence.
int pwpp_evidence_obstacles(pwpp_handle *h, const pwpp_ground_grid *g, float h_min, float h_max, int min_count, int connectivity, int frame_first, int frames, int mem,
                            int32_t *label, int32_t *count, float *top, pwpp_obstacle_cluster *clusters, int32_t *n_clusters, int max_clusters, int32_t *point_cluster,
                            const int8_t *occupancy_in, const double *pose, int n_poses, const int32_t *map_of_frame, const pwpp_fusion_map *m, int n_maps,
                            const int16_t *map, const pwpp_evidence_rule *rule, pwpp_cluster_evidence *rows, int8_t *cell_class, int8_t *occupancy_out) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!g || !label || !pose || !m || !map || !rule || !rows)
        return fail(PWPP_E_ARG, "null %s",
                    !g ? "grid" : (!label ? "label image" : (!pose ? "pose" : (!m ? "map description" : (!map ? "map" : (!rule ? "rule" : "rows"))))));
    const LabelArrays l{label, count, top, clusters, n_clusters, max_clusters, point_cluster};
    size_t cells = 0;
    int rc = label_first_args(h, g, h_min, h_max, min_count, connectivity, frame_first, frames, mem, l, kEvidenceWho, cells);
    if (rc) return rc;
    if (g->flags != 0) return fail(PWPP_E_ARG, "grid flags %d: the map evidence's frame grid takes 0", g->flags);
    EvidencePlan plan;
    if ((rc = image_args(m->nx, m->ny, n_maps, kEvidenceWho, plan.map_cells))) return rc;
    const EvidenceArrays a{occupancy_in, pose, n_poses, map_of_frame, map, rows, cell_class, occupancy_out};
    if ((rc = evidence_args(g, frames, cells, label, a, m, n_maps, rule, max_clusters, plan))) return rc;
    if ((rc = evidence_alignment_args(mem, label, a))) return rc;
    return run_on_labels(h, g, h_min, h_max, min_count, connectivity, frame_first, frames, mem, cells, l, [&](Staging &st, int s_label) {
        const EvidenceSections es = evidence_sections(st, plan, frames, cells, s_label, a);
        return [&, es] { return evidence_launch(h, st, es, plan, frames, a); };
    });
}

// Host only: the verdict of a row, by the function the kernels use.
int pwpp_evidence_verdict(const pwpp_evidence_rule *rule, int32_t cells, int32_t landed, int32_t occupied, int32_t free_cells, int32_t *verdict) {
    if (!rule || !verdict) return fail(PWPP_E_ARG, "null %s", rule ? "verdict" : "rule");
    PwppEvidenceRule R;
    if (const int rc = evidence_rule_args(rule, R)) return rc;
    if (cells < 0 || landed < 0 || occupied < 0 || free_cells < 0 || landed > cells || (int64_t)occupied + (int64_t)free_cells > (int64_t)landed)
        return fail(PWPP_E_ARG, "counts cells %d, landed %d, occupied %d, free %d: 0 <= occupied + free <= landed <= cells expected", cells, landed, occupied, free_cells);
    *verdict = pwpp_evid_verdict(R, cells, landed, occupied, free_cells);
    return PWPP_OK;
}

// ---- obstacle boxes: the counted points of every label as an oriented box --------------------------------------------------------
namespace {
static_assert(sizeof(pwpp_obstacle_box) == 64 && alignof(pwpp_obstacle_box) == 4, "pwpp_obstacle_box is 64 bytes of 4-byte fields");
constexpr size_t kBoxRowWords = sizeof(pwpp_obstacle_box) / 4;
// What option "boxes_path" = 0 means: whether the lanes of a wave that name one row are combined before the atomics.  Decided by
// tools/obstacle_boxes_cost.py (profiles/obstacle_boxes_cost.txt), not in advance.
constexpr bool kBoxesDefaultCombine = false;

int box_extent_args(const pwpp_ground_grid *g) {
    if (!((double)g->nx * g->cell <= PWPP_BOX_MAX_EXTENT) || !((double)g->ny * g->cell <= PWPP_BOX_MAX_EXTENT))
        return fail(PWPP_E_ARG, "grid of %d x %d cells of %g m: the obstacle boxes take an extent of at most 1024 m", g->nx, g->ny, g->cell);
    return PWPP_OK;
}

// ---- the rows of a label image, boxes or hulls: stated once for both tables -----------------------------------------------------------
struct RowTableNouns {
    const char *table, *rows, *who;
};
constexpr RowTableNouns kBoxNouns = {"box table", "boxes", "the obstacle boxes take"}, kHullNouns = {"hull table", "hulls", "the obstacle hulls take"};

// What a table of max_rows rows a frame may be; `max_vertices`: the length of the hulls' vertex lists (null: a table without lists)
int row_table_args(int64_t frames, int max_rows, const char *rows, const int *max_vertices) {
    if (max_rows < 1) return fail(PWPP_E_ARG, "max_%s %d: at least 1 expected", rows, max_rows);
    if (max_vertices && (*max_vertices < 1 || *max_vertices > PWPP_HULL_MAX_VERTICES))
        return fail(PWPP_E_ARG, "max_vertices %d: 1 .. %d expected", *max_vertices, PWPP_HULL_MAX_VERTICES);
    if (frames > 0 && frames * (int64_t)max_rows > ((int64_t)1 << 24)) return fail(PWPP_E_ARG, "%lld frames x %d %s exceed 2^24 rows", (long long)frames, max_rows, rows);
    if (max_vertices && frames > 0 && frames * (int64_t)max_rows * (int64_t)*max_vertices > ((int64_t)1 << 28))
        return fail(PWPP_E_ARG, "%lld frames x %d %s x %d vertices exceed 2^28", (long long)frames, max_rows, rows, *max_vertices);
    return PWPP_OK;
}

// What pwpp_box_obstacles and pwpp_hull_obstacles check first, in this order (the hulls' table, of 64-bit words: its alignment too); lands the call in flight.
int row_table_obstacle_args(pwpp_handle *h, const pwpp_ground_grid *g, float h_min, float h_max, int frame_first, int frames, int mem, const int32_t *label,
                            const void *table, int max_rows, const int *max_vertices, const RowTableNouns &n, size_t &cells) {
    if (!h) return fail(PWPP_E_ARG, "null handle");
    if (!g || !label || !table) return fail(PWPP_E_ARG, "null %s", !g ? "grid" : (!label ? "label image" : n.table));
    int rc = obstacle_band_args(g, h_min, h_max);
    if (rc || (rc = row_table_args(frames, max_rows, n.rows, max_vertices)) || (rc = box_extent_args(g)) || (rc = mem_args(mem, n.who))) return rc;
    if (max_vertices && (rc = alignment_args(mem, {{table, 7u, n.table}}))) return rc;
    return (rc = ground_grid_args(h, g, frame_first, frames, mem, cells)) ? rc : frame_cells_args(g->nx, g->ny);
}

// The five launches both end in: the rows' step 0, then for each of the two point passes the pass and the rows' step 1 + pass; the first failing code.
extern "C++" template <class Rows, class Pass>  // (the entry points' extern "C" block is open around this namespace)
int row_table_launches(Rows rows, Pass pass) {
    int lrc = rows(0);
    for (int p = 0; p < 2 && lrc == 0; ++p)
        if ((lrc = pass(p)) == 0) lrc = rows(1 + p);
    return lrc;
}

// Whether the raster counts a point at (x, y): the cell rule as pwpp_vis_cell_of states it (grid_cell of pwpp_kernels.hip: the same rule with a float input) ...
bool grid_counts(const pwpp_ground_grid *g, float x, float y) {
    int cell = 0;
    return pwpp_vis_cell_of((double)x, g->x0, g->cell, g->nx, cell) && pwpp_vis_cell_of((double)y, g->y0, g->cell, g->ny, cell);
}
// ... and the points of a caller's list a table's host form counts: the row in [0, max_rows), counted(i) (its NaN rule), inside the
// grid.  visit(i, row, dx, dy): the point's offsets from the grid's origin, in double.
extern "C++" template <class Counted, class Visit>
void counted_points(const pwpp_ground_grid *g, const float *xyz, const int32_t *row, int64_t m, int max_rows, Counted counted, Visit visit) {
    for (int64_t i = 0; i < m; ++i)
        if (row[i] >= 0 && row[i] < max_rows && counted(i) && grid_counts(g, xyz[3 * i], xyz[3 * i + 1]))
            visit(i, row[i], (double)xyz[3 * i] - g->x0, (double)xyz[3 * i + 1] - g->y0);
}
}  // namespace

// Init, first pass, solve, second pass, finish: five launches on the handle's stream.  The accumulators, and for PWPP_MEM_HOST the
// label image and the rows, live in the cluster buffer.
int pwpp_box_obstacles(pwpp_handle *h, const pwpp_ground_grid *g, float h_min, float h_max, int frame_first, int frames, int mem, const int32_t *label,
                       pwpp_obstacle_box *boxes, int max_boxes) {
    size_t cells = 0;
    int rc = row_table_obstacle_args(h, g, h_min, h_max, frame_first, frames, mem, label, boxes, max_boxes, nullptr, kBoxNouns, cells);
    if (rc) return rc;
    const size_t rows = (size_t)frames * (size_t)max_boxes;
    Staging st(h, h->d_clusters, mem, kClusterAlign);
    const int s_acc = st.add(rows * PWPP_BOX_ACC_WORDS, nullptr, Staging::kKept);
    const int s_label = st.add(cells, label, Staging::kIn), s_rows = st.add(rows * kBoxRowWords, boxes, Staging::kOut);
    if ((rc = st.begin())) return rc;
    PwppObstacleScan scan;
    if ((rc = obstacle_scan(h, g, h_min, h_max, frame_first, frames, scan))) return rc;
    const PwppBoxRows table = {st.dev<const int32_t>(s_label), max_boxes, st.dev<uint32_t>(s_acc), st.dev<const float>(s_rows)};
    const int combine = h->boxes_path == 0 ? (kBoxesDefaultCombine ? 1 : 0) : (h->boxes_path == 2 ? 1 : 0);
    const int lrc = row_table_launches([&](int step) { return pwpp_launch_box_rows(step, (int64_t)rows, table.acc, g->x0, g->y0, st.dev<void>(s_rows), h->stream); },
                                       [&](int pass) { return pwpp_launch_box_pass(pass, combine, &scan, &table, h->stream); });
    return lrc != 0 ? launch_failed(h, lrc) : st.end();
}

// The same rows on the host, from the functions the kernels compile (pwpp_boxes.h); row and height of every point are the caller's.
int pwpp_box_points(const pwpp_ground_grid *g, const float *xyz, const float *hgt, const int32_t *row, int64_t m, pwpp_obstacle_box *boxes, int max_boxes) {
    if (!g || !boxes) return fail(PWPP_E_ARG, "null %s", g ? "box table" : "grid");
    if (max_boxes < 1 || max_boxes > (1 << 24)) return fail(PWPP_E_ARG, "max_boxes %d: 1 .. 2^24 expected", max_boxes);
    if (m < 0 || m > ((int64_t)1 << 22)) return fail(PWPP_E_ARG, "%lld points (0..2^22 supported)", (long long)m);
    if (m > 0 && (!xyz || !hgt || !row)) return fail(PWPP_E_ARG, "null %s", !xyz ? "positions" : (!hgt ? "heights" : "rows"));
    int rc = grid_geometry_args(g);
    if (rc || (rc = box_extent_args(g))) return rc;
    struct Acc {
        long long s[PWPP_BOX_SUMS];
        uint32_t k[PWPP_BOX_KEYS];
    };
    Acc empty;
    for (int j = 0; j < PWPP_BOX_SUMS; ++j) empty.s[j] = 0;
    for (int j = 0; j < PWPP_BOX_KEYS; ++j) empty.k[j] = (j & 1) ? PWPP_BOX_KEY_NO_MAX : PWPP_BOX_KEY_NO_MIN;
    std::vector<Acc> acc((size_t)max_boxes, empty);
    std::vector<PwppBoxAxis> axis((size_t)max_boxes, PwppBoxAxis{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f});
    for (int pass = 0; pass < 2; ++pass) {
        counted_points(g, xyz, row, m, max_boxes, [&](int64_t i) { return hgt[i] == hgt[i]; }, [&](int64_t i, int32_t r, double dx, double dy) {
            Acc &a = acc[(size_t)r];
            if (pass == 0) {
                const long long qx = pwpp_box_quantise(dx), qy = pwpp_box_quantise(dy);
                a.s[0] += 1, a.s[1] += qx, a.s[2] += qy, a.s[3] += qx * qx, a.s[4] += qx * qy, a.s[5] += qy * qy;
            } else {
                float p, q;
                pwpp_box_project(dx, dy, axis[(size_t)r].ax, axis[(size_t)r].ay, p, q);
                const uint32_t k[4] = {pwpp_height_key(p), pwpp_height_key(q), pwpp_height_key(hgt[i]), pwpp_height_key(xyz[3 * i + 2])};
                for (int j = 0; j < 4; ++j) {
                    a.k[2 * j] = std::min(a.k[2 * j], k[j]);
                    a.k[2 * j + 1] = std::max(a.k[2 * j + 1], k[j]);
                }
            }
        });
        for (int r = 0; r < max_boxes; ++r) {
            const Acc &a = acc[(size_t)r];
            if (pass == 0) {
                if (a.s[0] > 0) axis[(size_t)r] = pwpp_box_solve(a.s[0], a.s[1], a.s[2], a.s[3], a.s[4], a.s[5], g->x0, g->y0);
            } else {
                uint32_t out[16];
                pwpp_box_row(a.s[0], axis[(size_t)r], a.k, g->x0, g->y0, out);
                std::memcpy(&boxes[r], out, sizeof(out));
            }
        }
    }
    return PWPP_OK;
}

// ---- obstacle hulls: the counted points of every label as a convex hull and its tightest rectangle ---------------------------------
namespace {
static_assert(sizeof(pwpp_obstacle_hull) == 64 && alignof(pwpp_obstacle_hull) == 8 && offsetof(pwpp_obstacle_hull, area2) == 16 &&
                  offsetof(pwpp_obstacle_hull, qx_min) == 24 && offsetof(pwpp_obstacle_hull, cx) == 40,
              "pwpp_obstacle_hull is the sixteen words of pwpp_hull_row");
static_assert(sizeof(pwpp_obstacle_hull) / 4 == PWPP_HULL_ROW_WORDS && PWPP_HULL_VERTICES_MAX == PWPP_HULL_MAX_VERTICES, "the kernels' row and vertex limit");
}  // namespace

// Init, first pass, offsets, second pass, rows: five launches on the handle's stream.  The accumulators, the candidate arena, the
// vertex lists nobody asked for (path 1 reads them back) and for PWPP_MEM_HOST the caller's arrays live in the cluster buffer.
int pwpp_hull_obstacles(pwpp_handle *h, const pwpp_ground_grid *g, float h_min, float h_max, int frame_first, int frames, int mem, const int32_t *label,
                        pwpp_obstacle_hull *hulls, int max_hulls, int32_t *vertices, int max_vertices) {
    size_t cells = 0;
    int rc = row_table_obstacle_args(h, g, h_min, h_max, frame_first, frames, mem, label, hulls, max_hulls, &max_vertices, kHullNouns, cells);
    if (rc) return rc;
    PwppObstacleScan scan;
    if ((rc = obstacle_scan(h, g, h_min, h_max, frame_first, frames, scan))) return rc;
    const int path = pwpp_hull_path_of(h->hulls_path, (int64_t)frames * (int64_t)max_hulls);
    const size_t rows = (size_t)frames * (size_t)max_hulls, lists = rows * (size_t)max_vertices * 2;
    const size_t arena = (size_t)frames * (size_t)scan.max_nonground * 2;  // (8 bytes an entry: PWPP_HULL_ARENA_BYTES of the header)
    Staging st(h, h->d_clusters, mem, kClusterAlign);
    const int s_acc = st.add(rows * PWPP_HULL_ACC_WORDS, nullptr, Staging::kKept), s_arena = st.add(arena, nullptr, Staging::kKept);
    const int s_label = st.add(cells, label, Staging::kIn), s_rows = st.add(rows * PWPP_HULL_ROW_WORDS, hulls, Staging::kOut);
    const int s_lists = vertices ? st.add(lists, vertices, Staging::kOut) : st.add(path == 1 ? lists : 0, nullptr, Staging::kKept);
    if ((rc = st.begin())) return rc;
    const PwppHullRows table = {st.dev<const int32_t>(s_label), max_hulls, st.dev<uint32_t>(s_acc), st.dev<unsigned long long>(s_arena), (int64_t)scan.max_nonground};
    int32_t *d_lists = (vertices || path == 1) ? st.dev<int32_t>(s_lists) : nullptr;
    const int lrc = row_table_launches(
        [&](int step) { return pwpp_launch_hull_rows(step, path, frames, &table, g->x0, g->y0, st.dev<void>(s_rows), d_lists, max_vertices, h->stream); },
        [&](int pass) { return pwpp_launch_hull_pass(pass, &scan, &table, h->stream); });
    return lrc != 0 ? launch_failed(h, lrc) : st.end();
}

// The same rows on the host, from the functions the kernels compile (pwpp_hull.h): every point of a row is a candidate.
int pwpp_hull_points(const pwpp_ground_grid *g, const float *xyz, const int32_t *row, int64_t m, pwpp_obstacle_hull *hulls, int max_hulls, int32_t *vertices,
                     int max_vertices) {
    if (!g || !hulls) return fail(PWPP_E_ARG, "null %s", g ? "hull table" : "grid");
    int rc = row_table_args(1, max_hulls, kHullNouns.rows, &max_vertices);
    if (rc) return rc;
    if (m < 0 || m > ((int64_t)1 << 22)) return fail(PWPP_E_ARG, "%lld points (0..2^22 supported)", (long long)m);
    if (m > 0 && (!xyz || !row)) return fail(PWPP_E_ARG, "null %s", !xyz ? "positions" : "rows");
    if ((rc = grid_geometry_args(g)) || (rc = box_extent_args(g))) return rc;
    try {
        std::vector<int64_t> first((size_t)max_hulls + 1, 0);
        std::vector<int32_t> of;  // the row of every counted point, -1: skipped
        of.assign((size_t)m, -1);
        std::vector<pwpp_hull_pt> pt((size_t)m, 0);
        counted_points(g, xyz, row, m, max_hulls, [&](int64_t i) { return xyz[3 * i + 2] == xyz[3 * i + 2]; }, [&](int64_t i, int32_t r, double dx, double dy) {
            of[(size_t)i] = r, pt[(size_t)i] = pwpp_hull_pack(pwpp_box_quantise(dx), pwpp_box_quantise(dy));
            first[(size_t)r + 1] += 1;
        });
        for (int r = 0; r < max_hulls; ++r) first[(size_t)r + 1] += first[(size_t)r];
        std::vector<pwpp_hull_pt> cand((size_t)first[(size_t)max_hulls], 0);
        std::vector<int64_t> at(first.begin(), first.end() - 1);
        for (int64_t i = 0; i < m; ++i)
            if (of[(size_t)i] >= 0) cand[(size_t)at[(size_t)of[(size_t)i]]++] = pt[(size_t)i];
        std::vector<int32_t> own(vertices ? 0 : (size_t)max_vertices * 2, 0);
        for (int r = 0; r < max_hulls; ++r) {
            const int64_t n = first[(size_t)r + 1] - first[(size_t)r];
            uint32_t out[PWPP_HULL_ROW_WORDS];
            pwpp_hull_row_serial(cand.data() + first[(size_t)r], n, (int32_t)n, max_vertices, vertices ? vertices + (size_t)r * (size_t)max_vertices * 2 : own.data(), g->x0,
                                 g->y0, out);
            std::memcpy(&hulls[r], out, sizeof(out));
        }
    } catch (const std::bad_alloc &) {
        return fail(PWPP_E_NOMEM, "no host memory for %lld points and %d rows", (long long)m, max_hulls);
    }
    return PWPP_OK;
}

int pwpp_hull_vertex_xy(const pwpp_ground_grid *g, const int32_t *q, double *out) {
    if (!g || !q || !out) return fail(PWPP_E_ARG, "null %s", !g ? "grid" : (!q ? "vertex" : "output"));
    out[0] = (double)(g->x0 + (double)q[0] / 1024.0);
    out[1] = (double)(g->y0 + (double)q[1] / 1024.0);
    return PWPP_OK;
}

int pwpp_set_overlap(pwpp_handle *h, int on) {
    int rc = enter(h);
    if (rc) return rc;
    h->overlap = on != 0;
    return PWPP_OK;
}

int pwpp_get_one_pass_stats(pwpp_handle *h, int64_t *batches, int64_t *redone) {
    int rc = enter(h);
    if (rc) return rc;
    if (batches) *batches = h->one_pass_batches;
    if (redone) *redone = h->one_pass_redone;
    return PWPP_OK;
}

int pwpp_get_arena_stats(pwpp_handle *h, int64_t *frames_with_moved_parts, int64_t *slots_per_frame, int64_t *arena_slots) {
    int rc = enter(h);
    if (rc) return rc;
    if (frames_with_moved_parts) *frames_with_moved_parts = h->arena_frames;
    if (slots_per_frame) *slots_per_frame = h->slots_per_frame;
    if (arena_slots) *arena_slots = h->arena_slots;
    return PWPP_OK;
}

int pwpp_get_redo_stats(pwpp_handle *h, int64_t *frames_one_pass, int64_t *frames_redone) {
    int rc = enter(h);
    if (rc) return rc;
    if (frames_one_pass) *frames_one_pass = h->one_pass_frames;
    if (frames_redone) *frames_redone = h->one_pass_redone_frames;
    return PWPP_OK;
}

/* timing probes of the last call (PWPP_DEBUG_FLAGS & 4) */
int pwpp_debug_read(pwpp_handle *h, unsigned long long *out64) {
    if (!h || !out64) return fail(PWPP_E_ARG, "null argument");
    int rc = enter(h);
    if (rc) return rc;
    if (!h->d_dbg.p) return fail(PWPP_E_STATE, "no probes");
    HIPCHK(hipMemcpy(out64, h->d_dbg.p, 64 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return PWPP_OK;
}


/* ---- batches in flight (include/pwpp.h) ---- */
struct pwpp_pipe {
    std::vector<pwpp_handle *> handles;
    unsigned long long submits = 0;
};

int pwpp_pipe_create(const pwpp_params *p, int device, int depth, pwpp_pipe **out) {
    if (!p || !out) return fail(PWPP_E_ARG, "null argument");
    if (depth < 1 || depth > 4) return fail(PWPP_E_ARG, "depth %d: 1..4 expected", depth);
    pwpp_pipe *pipe = new (std::nothrow) pwpp_pipe;
    if (!pipe) return fail(PWPP_E_NOMEM, "out of host memory");
    for (int k = 0; k < depth; ++k) {
        pwpp_handle *h = nullptr;
        const int rc = pwpp_create(p, device, &h);
        if (rc) {
            (void)pwpp_pipe_destroy(pipe);
            return rc;
        }
        if (depth > 1) h->overlap = false;  // (the in-handle overlap schedule on top of batches in flight is slower: 2.83 against 2.46 ms)
        pipe->handles.push_back(h);
    }
    *out = pipe;
    return PWPP_OK;
}

int pwpp_pipe_set_num_streams(pwpp_pipe *pipe, int streams_per_handle) {
    if (!pipe || pipe->handles.empty()) return fail(PWPP_E_ARG, "null pipe");
    for (pwpp_handle *h : pipe->handles) {
        const int rc = pwpp_set_num_streams(h, streams_per_handle);
        if (rc) return rc;
    }
    return PWPP_OK;
}

int pwpp_pipe_submit(pwpp_pipe *pipe, const float *const *points, const int32_t *n, int frames, int cols, int layout, int mem, int mode,
                     pwpp_handle **holder) {
    if (!pipe || pipe->handles.empty()) return fail(PWPP_E_ARG, "null pipe");
    pwpp_handle *h = pipe->handles[(size_t)(pipe->submits % pipe->handles.size())];
    // (pwpp_estimate_ground_batch first waits for this handle's own batch in flight: the one submitted `depth` submits ago.
    // PWPP_MODE_STREAMS: the handle owns the streams of ITS group -- submit k carries group k mod depth, so a stream's frames
    // stay in order on one handle; the mode is checked there, together with the stream count)
    const int rc = pwpp_estimate_ground_batch(h, points, n, frames, cols, layout, mem, mode);
    if (rc) return rc;
    ++pipe->submits;
    if (holder) *holder = h;
    return PWPP_OK;
}

int pwpp_pipe_drain(pwpp_pipe *pipe) {
    if (!pipe) return fail(PWPP_E_ARG, "null pipe");
    for (pwpp_handle *h : pipe->handles) {
        const int rc = pwpp_synchronize(h);
        if (rc) return rc;
    }
    return PWPP_OK;
}

pwpp_handle *pwpp_pipe_handle(pwpp_pipe *pipe, int index) {
    return pipe && index >= 0 && (size_t)index < pipe->handles.size() ? pipe->handles[(size_t)index] : nullptr;
}

int pwpp_pipe_destroy(pwpp_pipe *pipe) {
    if (!pipe) return PWPP_OK;
    int rc = PWPP_OK;
    for (pwpp_handle *h : pipe->handles) {
        const int r = pwpp_destroy(h);
        rc = rc ? rc : r;
    }
    delete pipe;
    return rc;
}

}  // extern "C"
