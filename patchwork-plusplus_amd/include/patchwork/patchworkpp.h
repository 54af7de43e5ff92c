// patchwork/patchworkpp.h -- host-side C++ mirror of the reference's public interface for the
// estimateGround() path, backed by the MI355X library (include/pwpp.h, libpwpp_hip.so).
//
// Mirrors /root/reference/cpp/patchworkpp/include/patchwork/patchworkpp.h:
//   patchwork::Params        (:42-112)  same field names, types and defaults
//   patchwork::PatchWorkpp   (:114-163) same constructor, estimateGround(), and getters
// so that code written against the reference header compiles against this one (see
// INTEGRATION.md).  Eigen is optional here (the container / no-network build has none):
//  * with <Eigen/Dense> on the include path the class has the reference's EXACT signatures --
//    estimateGround(Eigen::MatrixXf), getGround() etc. return real Eigen::MatrixX3f / Eigen::VectorXi
//    objects, so `pw.getGround().row(i)`, `.transpose()`, `auto g = pw.getNormals(); g.col(2)` compile
//    as against the reference;
//  * without it (or with PWPP_NO_EIGEN) the getters return the small row-major containers below and
//    estimateGround takes a raw pointer.
//
// Differences a caller can observe, all documented in DESIGN.md section 7 and INTEGRATION.md section 5:
//  * index and point lists hold the same SETS as the reference, ordered by the device
//    pipeline, not by the reference's bin traversal / z order;
//  * getTimeTaken() is GPU time in microseconds (the reference reports CPU clock ticks = us);
//  * errors throw std::runtime_error instead of printing.
#ifndef PATCHWORKPP_AMD_H
#define PATCHWORKPP_AMD_H

#include <cmath>
#include <cstdint>
#include <cstring>
#include <iostream>
#include <limits>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "pwpp.h"

#if defined(__has_include)
#if __has_include(<Eigen/Dense>) && !defined(PWPP_NO_EIGEN)
#include <Eigen/Dense>
#define PWPP_HAVE_EIGEN 1
#endif
#endif

namespace patchwork {

// reference patchworkpp.h:42-112
struct Params {
    bool verbose;
    bool enable_RNR;
    bool enable_RVPF;
    bool enable_TGR;

    int num_iter;
    int num_lpr;
    int num_min_pts;
    int num_zones;
    int num_rings_of_interest;

    double RNR_ver_angle_thr;
    double RNR_intensity_thr;

    double sensor_height;
    double th_seeds;
    double th_dist;
    double th_seeds_v;
    double th_dist_v;
    double max_range;
    double min_range;
    double uprightness_thr;
    double adaptive_seed_selection_margin;
    double intensity_thr;

    std::vector<int> num_sectors_each_zone;
    std::vector<int> num_rings_each_zone;

    int max_flatness_storage;
    int max_elevation_storage;

    std::vector<double> elevation_thr;
    std::vector<double> flatness_thr;

    Params() {
        verbose = false;
        enable_RNR = true;
        enable_RVPF = true;
        enable_TGR = true;

        num_iter = 3;
        num_lpr = 20;
        num_min_pts = 10;
        num_zones = 4;
        num_rings_of_interest = 4;

        RNR_ver_angle_thr = -15.0;
        RNR_intensity_thr = 0.2;

        sensor_height = 1.723;
        th_seeds = 0.125;
        th_dist = 0.125;
        th_seeds_v = 0.25;
        th_dist_v = 0.1;
        max_range = 80.0;
        min_range = 2.7;
        uprightness_thr = 0.707;
        adaptive_seed_selection_margin = -1.2;
        intensity_thr = 0.0;  // left uninitialised by the reference (:67); never read by the path

        num_sectors_each_zone = {16, 32, 54, 32};
        num_rings_each_zone = {2, 4, 4, 4};

        max_flatness_storage = 1000;
        max_elevation_storage = 1000;
        elevation_thr = {0, 0, 0, 0};
        flatness_thr = {0, 0, 0, 0};
    }
};

// Row-major (rows, 3) float container returned by getGround()/getNonground()/getCenters()/getNormals().
class Cloud {
public:
    Cloud() : rows_(0) {}
    explicit Cloud(int rows) : rows_(rows), v_((size_t)rows * 3) {}
    int rows() const { return rows_; }
    int cols() const { return 3; }
    float operator()(int i, int j) const { return v_[(size_t)i * 3 + j]; }
    float *data() { return v_.data(); }
    const float *data() const { return v_.data(); }
#ifdef PWPP_HAVE_EIGEN
    operator Eigen::MatrixX3f() const {
        Eigen::MatrixX3f m(rows_, 3);
        for (int i = 0; i < rows_; ++i)
            for (int j = 0; j < 3; ++j) m(i, j) = (*this)(i, j);
        return m;
    }
#endif
private:
    int rows_;
    std::vector<float> v_;
};

class Indices {
public:
    Indices() {}
    explicit Indices(int rows) : v_((size_t)rows) {}
    int rows() const { return (int)v_.size(); }
    int operator()(int i) const { return v_[(size_t)i]; }
    int32_t *data() { return v_.data(); }
    const int32_t *data() const { return v_.data(); }
#ifdef PWPP_HAVE_EIGEN
    operator Eigen::VectorXi() const {
        Eigen::VectorXi m(rows());
        for (int i = 0; i < rows(); ++i) m(i) = v_[(size_t)i];
        return m;
    }
#endif
private:
    std::vector<int32_t> v_;
};

// one PWPP_LABEL_* byte per point (getLabels without Eigen)
class Labels {
public:
    Labels() {}
    explicit Labels(int rows) : v_((size_t)rows) {}
    int rows() const { return (int)v_.size(); }
    uint8_t operator()(int i) const { return v_[(size_t)i]; }
    uint8_t *data() { return v_.data(); }
    const uint8_t *data() const { return v_.data(); }
private:
    std::vector<uint8_t> v_;
};

// one float per point (getPointDistances without Eigen)
class Distances {
public:
    Distances() {}
    explicit Distances(int rows) : v_((size_t)rows) {}
    int rows() const { return (int)v_.size(); }
    float operator()(int i) const { return v_[(size_t)i]; }
    float *data() { return v_.data(); }
    const float *data() const { return v_.data(); }
private:
    std::vector<float> v_;
};

// Row-major (rows, cols) floats: whole input rows, intensity included (getGroundPoints without Eigen)
class Points {
public:
    Points() : rows_(0), cols_(0) {}
    Points(int rows, int cols) : rows_(rows), cols_(cols), v_((size_t)rows * (size_t)cols) {}
    int rows() const { return rows_; }
    int cols() const { return cols_; }
    float operator()(int i, int j) const { return v_[(size_t)i * (size_t)cols_ + (size_t)j]; }
    float *data() { return v_.data(); }
    const float *data() const { return v_.data(); }
private:
    int rows_, cols_;
    std::vector<float> v_;
};

// reference patchworkpp.h:114-163
class PatchWorkpp {
public:
    PatchWorkpp(patchwork::Params _params, int device = 0) : params_(_params), h_(nullptr) {
        pwpp_params p;
        pwpp_params_default(&p);
        p.verbose = params_.verbose;
        p.enable_RNR = params_.enable_RNR;
        p.enable_RVPF = params_.enable_RVPF;
        p.enable_TGR = params_.enable_TGR;
        p.num_iter = params_.num_iter;
        p.num_lpr = params_.num_lpr;
        p.num_min_pts = params_.num_min_pts;
        p.num_zones = params_.num_zones;
        p.num_rings_of_interest = params_.num_rings_of_interest;
        p.RNR_ver_angle_thr = params_.RNR_ver_angle_thr;
        p.RNR_intensity_thr = params_.RNR_intensity_thr;
        p.sensor_height = params_.sensor_height;
        p.th_seeds = params_.th_seeds;
        p.th_dist = params_.th_dist;
        p.th_seeds_v = params_.th_seeds_v;
        p.th_dist_v = params_.th_dist_v;
        p.max_range = params_.max_range;
        p.min_range = params_.min_range;
        p.uprightness_thr = params_.uprightness_thr;
        p.adaptive_seed_selection_margin = params_.adaptive_seed_selection_margin;
        p.intensity_thr = params_.intensity_thr;
        // the reference constructor reads .at(0..3) of both vectors (:127-134) and indexes
        // elevation_thr / flatness_thr up to num_rings_of_interest (patchworkpp.cpp:244-245)
        for (int k = 0; k < 4; ++k) {
            p.num_sectors_each_zone[k] = params_.num_sectors_each_zone.at((size_t)k);
            p.num_rings_each_zone[k] = params_.num_rings_each_zone.at((size_t)k);
            p.elevation_thr[k] = (size_t)k < params_.elevation_thr.size() ? params_.elevation_thr[(size_t)k] : 0.0;
            p.flatness_thr[k] = (size_t)k < params_.flatness_thr.size() ? params_.flatness_thr[(size_t)k] : 0.0;
        }
        p.max_flatness_storage = params_.max_flatness_storage;
        p.max_elevation_storage = params_.max_elevation_storage;
        p.verbose = 0;  // the line below is this class' job
        check(pwpp_create(&p, device, &h_));
        std::cout << "PatchWorkpp::PatchWorkpp() - INITIALIZATION COMPLETE" << std::endl;  // reference :149
    }
    ~PatchWorkpp() { pwpp_destroy(h_); }
    PatchWorkpp(const PatchWorkpp &) = delete;
    PatchWorkpp &operator=(const PatchWorkpp &) = delete;

    // estimateGround, reference patchworkpp.cpp:151.  `data` is rows x cols float32, cols = 3 or 4.
    void estimateGround(const float *data, int rows, int cols, bool row_major = true) {
        if (params_.verbose) check(pwpp_set_profiling(h_, 1));
        check(pwpp_estimate_ground(h_, data, rows, cols, row_major ? PWPP_LAYOUT_ROW_MAJOR : PWPP_LAYOUT_COL_MAJOR));
        if (params_.verbose) report_times();
    }
#ifdef PWPP_HAVE_EIGEN
    void estimateGround(Eigen::MatrixXf cloud_in) {  // the reference's exact signature
        estimateGround(cloud_in.data(), (int)cloud_in.rows(), (int)cloud_in.cols(), false);
    }
#endif

    double getHeight() { return pwpp_get_height(h_); }      // reference :154
    double getTimeTaken() { return pwpp_get_time_us(h_); }  // reference :155 (microseconds)
    // extension: true = the points of a patch come out in the reference's own order (bins sorted by z,
    // patchworkpp.cpp:199) instead of the scatter order; same sets either way (pwpp.h, pwpp_set_output_order)
    void setReferenceOrder(bool on) { check(pwpp_set_output_order(h_, on ? PWPP_ORDER_REFERENCE : PWPP_ORDER_SCATTER)); }
    // extension: true = both index lists in ascending cloud index (implies labels); false = scatter order
    void setCloudOrder(bool on) { check(pwpp_set_output_order(h_, on ? PWPP_ORDER_CLOUD : PWPP_ORDER_SCATTER)); }
    // extension: one PWPP_LABEL_* per point of the frames estimated afterwards (getLabels)
    void setLabels(bool on) { check(pwpp_set_labels(h_, on ? 1 : 0)); }
#if defined(PWPP_HAVE_EIGEN) && defined(EIGEN_WORLD_VERSION)  // (a partial Eigen API without Eigen::Matrix gets Labels)
    Eigen::Matrix<uint8_t, Eigen::Dynamic, 1> getLabels() {
        const Labels l = labels();
        Eigen::Matrix<uint8_t, Eigen::Dynamic, 1> m(l.rows());
        for (int i = 0; i < l.rows(); ++i) m(i) = l(i);
        return m;
    }
#else
    Labels getLabels() { return labels(); }
#endif
    Labels labelList() { return labels(); }
    // extension: per point of the frames estimated afterwards, the row of its patch in getCenters() / getNormals() (-1: none)
    // and its signed distance to that patch's plane (NaN: none); pwpp.h, pwpp_set_point_planes
    void setPointPlanes(bool on) { check(pwpp_set_point_planes(h_, on ? 1 : 0)); }
#ifdef PWPP_HAVE_EIGEN
    Eigen::VectorXi getPointPatches() {
        const Indices v = pointPatches();
        Eigen::VectorXi m(v.rows());
        for (int i = 0; i < v.rows(); ++i) m(i) = v(i);
        return m;
    }
    Eigen::VectorXf getPointDistances() {
        const Distances v = pointDistances();
        Eigen::VectorXf m(v.rows());
        for (int i = 0; i < v.rows(); ++i) m(i) = v(i);
        return m;
    }
#else
    Indices getPointPatches() { return pointPatches(); }
    Distances getPointDistances() { return pointDistances(); }
#endif
    Indices pointPatchList() { return pointPatches(); }
    Distances pointDistanceList() { return pointDistances(); }
    // extension: the frames estimated afterwards also leave the whole rows of their ground / non-ground points on the device
    // (pwpp.h, pwpp_set_point_records); getGroundPoints / getNongroundPoints work either way, and gather on demand without it
    void setPointRecords(bool on) { check(pwpp_set_point_records(h_, on ? 1 : 0)); }
    // extension: an affine transform [R | t] (3 x 4 row-major) applied to every point of the frames estimated afterwards, while
    // they are binned (pwpp.h, pwpp_set_input_transforms): a tilted mount, millimetres, an IMU's levelling.  getGround() /
    // getNonground(), centers, normals and queryGround() then live in the transformed frame; getGroundPoints() /
    // getNongroundPoints() stay the input rows.  nullptr turns it off.
    void setInputTransform(const float T[12]) { check(pwpp_set_input_transforms(h_, T, T ? 1 : 0)); }
    // getGround() / getNonground() with every column of the input: (count, cols) floats, rows aligned with the index getters
#ifdef PWPP_HAVE_EIGEN
    Eigen::MatrixXf getGroundPoints() { return to_eigen(points(true)); }
    Eigen::MatrixXf getNongroundPoints() { return to_eigen(points(false)); }
#else
    Points getGroundPoints() { return points(true); }
    Points getNongroundPoints() { return points(false); }
#endif
    Points groundPointRows() { return points(true); }
    Points nongroundPointRows() { return points(false); }
    // extension: the fitted ground model of the last frame at positions that are not cloud points (pwpp.h, pwpp_query_ground):
    // per position the row of its bin's patch in getCenters() / getNormals() (-1: none), that patch's decision, the height of
    // its plane at (x, y) and the signed distance of (x, y, z) to it.  `xyz`: m row-major (x, y, z) triples.
    std::vector<pwpp_ground_sample> queryGround(const float *xyz, int m) {
        std::vector<pwpp_ground_sample> out((size_t)(m > 0 ? m : 0));
        check(pwpp_query_ground(h_, xyz, nullptr, m, PWPP_MEM_HOST, out.data()));
        return out;
    }
    // ... and as a bird's-eye elevation image (pwpp_rasterize_ground): row iy, column ix = the plane height at the cell centre
    // (x0 + (ix + 0.5) cell, y0 + (iy + 0.5) cell), NaN where no patch answers; ground_only: NaN too where the patch was decided
    // not upright, heading or rejected by TGR
    Points elevationMapRows(double x0, double y0, double cell, int nx, int ny, bool ground_only = false) {
        const pwpp_ground_grid g = {x0, y0, cell, nx, ny, ground_only ? (int32_t)PWPP_GRID_GROUND_ONLY : 0, 0};
        Points img(ny > 0 ? ny : 0, nx > 0 ? nx : 0);
        float none = 0.0f;
        check(pwpp_rasterize_ground(h_, &g, 0, 1, PWPP_MEM_HOST, img.rows() > 0 && img.cols() > 0 ? img.data() : &none, nullptr));
        return img;
    }
    // ... and the other half of a 2.5-D map on the same grid (pwpp_rasterize_obstacles): per cell the number of non-ground points
    // whose height over their patch's plane lies in [h_min, h_max], and that largest height (NaN where the count is 0)
    struct ObstacleMap {
        std::vector<int32_t> count;  // ny x nx, row-major: row iy, column ix
        Points top;                  // (ny, nx)
    };
    ObstacleMap obstacleMapRows(double x0, double y0, double cell, int nx, int ny, float h_min, float h_max, bool ground_only = false) {
        const pwpp_ground_grid g = {x0, y0, cell, nx, ny, ground_only ? (int32_t)PWPP_GRID_GROUND_ONLY : 0, 0};
        ObstacleMap m;
        m.top = Points(ny > 0 ? ny : 0, nx > 0 ? nx : 0);
        m.count.assign((size_t)m.top.rows() * (size_t)m.top.cols(), 0);
        int32_t none_c = 0;
        float none_t = 0.0f;
        const bool any = !m.count.empty();
        check(pwpp_rasterize_obstacles(h_, &g, h_min, h_max, 0, 1, PWPP_MEM_HOST, any ? m.count.data() : &none_c, any ? m.top.data() : &none_t, nullptr));
        return m;
    }
    ObstacleMap getObstacleMap(double x0, double y0, double cell, int nx, int ny, float h_min, float h_max, bool ground_only = false) {
        return obstacleMapRows(x0, y0, cell, nx, ny, h_min, h_max, ground_only);
    }
    // ... and its occupied cells (count >= min_count) as connected clusters (pwpp_label_obstacles): per cell the rank of its
    // cluster in ascending first cell (-1: unoccupied), and per cluster the row of that rank -- cells, points, bounding box, top,
    // the sums of the point-weighted centroid.  connectivity: 4 (edges) or 8 (edges and corners).
    struct ObstacleClusters {
        std::vector<int32_t> label;                   // ny x nx, row-major: row iy, column ix
        std::vector<pwpp_obstacle_cluster> clusters;  // one row per cluster
        int count = 0;                                // clusters.size()
    };
    ObstacleClusters getObstacleClusters(double x0, double y0, double cell, int nx, int ny, float h_min, float h_max, int min_count = 1,
                                         int connectivity = 8, bool ground_only = false) {
        const pwpp_ground_grid g = {x0, y0, cell, nx, ny, ground_only ? (int32_t)PWPP_GRID_GROUND_ONLY : 0, 0};
        ObstacleClusters c;
        c.label.assign((size_t)(ny > 0 ? ny : 0) * (size_t)(nx > 0 ? nx : 0), -1);
        int32_t none = -1, n = 0;
        int32_t *label = c.label.empty() ? &none : c.label.data();
        // (the number of clusters first, then a table of exactly that many rows: the labels are the same both times)
        check(pwpp_label_obstacles(h_, &g, h_min, h_max, min_count, connectivity, 0, 1, PWPP_MEM_HOST, label, nullptr, nullptr, nullptr, &n, 0, nullptr));
        if (n > 0) {
            c.clusters.resize((size_t)n);
            check(pwpp_label_obstacles(h_, &g, h_min, h_max, min_count, connectivity, 0, 1, PWPP_MEM_HOST, label, nullptr, nullptr, c.clusters.data(), &n, n,
                                       nullptr));
        }
        c.count = n;
        return c;
    }
    // ... and every cell's distance to the nearest occupied cell (pwpp_distance_obstacles): the squared distance in cells
    // (PWPP_DIST_BEYOND: none in reach), the index iy * nx + ix of that cell (-1: none; the smallest among several) and the
    // distance in metres (+inf: none) -- an exact Euclidean distance transform, what a costmap inflater starts from.  max_dist > 0:
    // cells further than max_dist cells from every occupied cell report none.  clusters.label[nearest] is the nearest cluster.
    struct ObstacleDistances {
        std::vector<int32_t> dist2;    // ny x nx, row-major: row iy, column ix
        std::vector<int32_t> nearest;  // same shape
        Points metres;                 // (ny, nx)
    };
    ObstacleDistances getObstacleDistances(double x0, double y0, double cell, int nx, int ny, float h_min, float h_max, int min_count = 1, int max_dist = 0,
                                           bool ground_only = false) {
        const pwpp_ground_grid g = {x0, y0, cell, nx, ny, ground_only ? (int32_t)PWPP_GRID_GROUND_ONLY : 0, 0};
        ObstacleDistances d;
        d.metres = Points(ny > 0 ? ny : 0, nx > 0 ? nx : 0);
        d.dist2.assign((size_t)d.metres.rows() * (size_t)d.metres.cols(), PWPP_DIST_BEYOND);
        d.nearest.assign(d.dist2.size(), -1);
        int32_t none_d = 0, none_n = 0;
        float none_m = 0.0f;
        const bool any = !d.dist2.empty();
        check(pwpp_distance_obstacles(h_, &g, h_min, h_max, min_count, max_dist, 0, 1, PWPP_MEM_HOST, any ? d.dist2.data() : &none_d,
                                      any ? d.nearest.data() : &none_n, any ? d.metres.data() : &none_m, nullptr));
        return d;
    }
    // ... and the line-of-sight free space (pwpp_visibility_obstacles): for every cell the index iy * nx + ix of the first occupied
    // cell on the digital line from the sensor's cell (PWPP_VIS_NONE: the line is clear; PWPP_VIS_BEYOND: further than max_range >
    // 0 cells) and the tri-state byte of a nav_msgs/OccupancyGrid (PWPP_OCC_FREE, PWPP_OCC_OCCUPIED, PWPP_OCC_UNKNOWN).  The
    // sensor stands at (origin_x, origin_y) metres in the model's frame.  2-D line of sight on a 2.5-D map: a free cell behind a
    // low obstacle the sensor saw over is reported unknown.
    struct ObstacleVisibility {
        int nx = 0, ny = 0;
        std::vector<int32_t> first;     // ny x nx, row-major: row iy, column ix
        std::vector<int8_t> occupancy;  // same shape
    };
    ObstacleVisibility getObstacleVisibility(double x0, double y0, double cell, int nx, int ny, float h_min, float h_max, int min_count = 1,
                                             int max_range = 0, double origin_x = 0.0, double origin_y = 0.0, bool ground_only = false) {
        const pwpp_ground_grid g = {x0, y0, cell, nx, ny, ground_only ? (int32_t)PWPP_GRID_GROUND_ONLY : 0, 0};
        ObstacleVisibility v;
        v.nx = nx > 0 ? nx : 0, v.ny = ny > 0 ? ny : 0;
        v.first.assign((size_t)v.nx * (size_t)v.ny, PWPP_VIS_NONE);
        v.occupancy.assign(v.first.size(), (int8_t)PWPP_OCC_UNKNOWN);
        int32_t none_f = 0;
        int8_t none_o = 0;
        const double origin[2] = {origin_x, origin_y};
        const bool any = !v.first.empty();
        check(pwpp_visibility_obstacles(h_, &g, h_min, h_max, min_count, origin, 1, max_range, 0, 1, PWPP_MEM_HOST, any ? v.first.data() : &none_f,
                                        any ? v.occupancy.data() : &none_o, nullptr));
        return v;
    }
    // ... the same with heights (pwpp_viewshed_obstacles): an obstacle hides a cell only where the ray from the sensor at (origin_x,
    // origin_y, origin_z) metres to the cell's ground passes through it, and a cell whose ground sent min_seen returns back is free
    // (min_seen 0: ground returns are not used).  first: the nearest cell that hides; shadow: the lowest height seen at the cell in
    // units of 1 / PWPP_VIEW_UNITS_PER_M m (PWPP_VIEW_NO_HEIGHT: no obstacle on the line; INT32_MAX: behind an opaque one).
    struct ObstacleViewshed {
        int nx = 0, ny = 0;
        std::vector<int32_t> first;     // ny x nx, row-major: row iy, column ix
        std::vector<int32_t> shadow;    // same shape
        std::vector<int8_t> occupancy;  // same shape
    };
    ObstacleViewshed getObstacleViewshed(double x0, double y0, double cell, int nx, int ny, float h_min, float h_max, int min_count = 1, int min_seen = 1,
                                         int max_range = 0, double origin_x = 0.0, double origin_y = 0.0, double origin_z = 0.0, bool ground_only = false) {
        const pwpp_ground_grid g = {x0, y0, cell, nx, ny, ground_only ? (int32_t)PWPP_GRID_GROUND_ONLY : 0, 0};
        ObstacleViewshed v;
        v.nx = nx > 0 ? nx : 0, v.ny = ny > 0 ? ny : 0;
        v.first.assign((size_t)v.nx * (size_t)v.ny, PWPP_VIS_NONE);
        v.shadow.assign(v.first.size(), PWPP_VIEW_NO_HEIGHT);
        v.occupancy.assign(v.first.size(), (int8_t)PWPP_OCC_UNKNOWN);
        int32_t none_f = 0, none_s = 0;
        int8_t none_o = 0;
        const double origin[3] = {origin_x, origin_y, origin_z};
        const bool any = !v.first.empty();
        check(pwpp_viewshed_obstacles(h_, &g, h_min, h_max, min_count, min_seen, origin, 1, max_range, 0, 1, PWPP_MEM_HOST, any ? v.first.data() : &none_f,
                                      any ? v.shadow.data() : &none_s, any ? v.occupancy.data() : &none_o, nullptr));
        return v;
    }

    // ... and the free space the returns themselves prove (pwpp_beam_ground): the beam of every selected return (which:
    // PWPP_BEAMS_GROUND, PWPP_BEAMS_NONGROUND or both) is drawn from the sensor's cell to the return's cell.  passes: the beams that
    // crossed the cell; low: the lowest height, in units of 1 / PWPP_VIEW_UNITS_PER_M m, at which one crossed it (PWPP_VIEW_NO_HEIGHT:
    // none); occupancy: occupancy_in (empty: all unknown; else ny x nx bytes, typically getObstacleViewshed's) with every unknown
    // cell free that min_pass beams crossed no more than `clearance` metres above its ground.
    struct BeamClearance {
        int nx = 0, ny = 0;
        std::vector<uint32_t> passes;   // ny x nx, row-major: row iy, column ix
        std::vector<int32_t> low;       // same shape
        std::vector<int8_t> occupancy;  // same shape
    };
    BeamClearance getBeamClearance(double x0, double y0, double cell, int nx, int ny, int min_pass = 1, double clearance = 0.3, int max_range = 0,
                                   double origin_x = 0.0, double origin_y = 0.0, double origin_z = 0.0, int which = PWPP_BEAMS_GROUND, bool ground_only = false,
                                   const std::vector<int8_t> &occupancy_in = std::vector<int8_t>()) {
        const pwpp_ground_grid g = {x0, y0, cell, nx, ny, ground_only ? (int32_t)PWPP_GRID_GROUND_ONLY : 0, 0};
        BeamClearance v;
        v.nx = nx > 0 ? nx : 0, v.ny = ny > 0 ? ny : 0;
        v.passes.assign((size_t)v.nx * (size_t)v.ny, 0u);
        v.low.assign(v.passes.size(), PWPP_VIEW_NO_HEIGHT);
        v.occupancy.assign(v.passes.size(), (int8_t)PWPP_OCC_UNKNOWN);
        if (!occupancy_in.empty() && occupancy_in.size() != v.passes.size()) throw std::invalid_argument("getBeamClearance: occupancy_in must be ny x nx bytes");
        int32_t none_p = 0, none_l = 0;
        int8_t none_o = 0;
        const double origin[3] = {origin_x, origin_y, origin_z};
        const bool any = !v.passes.empty();
        check(pwpp_beam_ground(h_, &g, which, origin, 1, max_range, min_pass, clearance, 0, 1, PWPP_MEM_HOST, occupancy_in.empty() ? nullptr : occupancy_in.data(),
                               any ? reinterpret_cast<int32_t *>(v.passes.data()) : &none_p, any ? v.low.data() : &none_l, any ? v.occupancy.data() : &none_o,
                               nullptr, nullptr));
        return v;
    }
    // ... and the scans accumulated over time (pwpp_fuse_obstacles): a persistent map in a FIXED frame, the caller's own.  log_odds
    // holds an int16 per cell, occupancy the byte derived from it (PWPP_OCC_OCCUPIED where log_odds >= occupied_at, PWPP_OCC_FREE
    // where <= free_at, else PWPP_OCC_UNKNOWN).  updateObstacleMap resamples the last frame's visibility bytes on the grid (x0, y0,
    // cell, nx, ny) under the map-from-frame pose {a, b, tx, c, d, ty} and adds hit / subtracts miss with the clamps; (shift_x,
    // shift_y) cells roll the map first: the new cell (jx, jy) starts from the old (jx + shift_x, jy + shift_y), the map's x0 and
    // y0 advance by shift * cell.
    struct FusedObstacleMap {
        double x0 = 0.0, y0 = 0.0, cell = 0.0;  // the map's grid: cell (jx, jy) covers x0 + [jx, jx + 1) * cell, ...
        int nx = 0, ny = 0;
        int hit = 40, miss = 20, l_min = -200, l_max = 350, occupied_at = 60, free_at = -40;
        std::vector<int16_t> log_odds;  // ny x nx, row-major; sized and zeroed by the first update
        std::vector<int8_t> occupancy;  // same shape
    };
    void updateObstacleMap(FusedObstacleMap &map, const double pose[6], double x0, double y0, double cell, int nx, int ny, float h_min, float h_max,
                           int min_count = 1, int max_range = 0, double origin_x = 0.0, double origin_y = 0.0, int shift_x = 0, int shift_y = 0) {
        const pwpp_ground_grid g = {x0, y0, cell, nx, ny, 0, 0};
        const double mx0 = map.x0 + (double)shift_x * map.cell, my0 = map.y0 + (double)shift_y * map.cell;
        const pwpp_fusion_map m = {mx0, my0, map.cell, map.nx, map.ny, map.hit, map.miss, map.l_min, map.l_max, map.occupied_at, map.free_at};
        const size_t cells = (size_t)(map.nx > 0 ? map.nx : 0) * (size_t)(map.ny > 0 ? map.ny : 0);
        if (map.log_odds.size() != cells) map.log_odds.assign(cells, 0);
        std::vector<int16_t> out(cells ? cells : 1);
        map.occupancy.assign(cells ? cells : 1, (int8_t)PWPP_OCC_UNKNOWN);
        const double origin[2] = {origin_x, origin_y};
        const int32_t shift[2] = {shift_x, shift_y};
        check(pwpp_fuse_obstacles(h_, &g, h_min, h_max, min_count, origin, 1, max_range, 0, 1, PWPP_MEM_HOST, pose, 1, nullptr, &m, 1, shift,
                                  cells ? map.log_odds.data() : nullptr, out.data(), map.occupancy.data(), nullptr));
        out.resize(cells), map.occupancy.resize(cells);
        map.log_odds.swap(out);
        map.x0 = mx0, map.y0 = my0;
    }
    // ... and the ground under them accumulated the same way (pwpp_fuse_ground): a persistent elevation map in the same FIXED frame,
    // the caller's own.  sum holds an int32 per cell, the sum of the heights the cell remembers in units of 2^-10 m, n how many it
    // remembers (at most n_max; beyond that the mean forgets one share of itself per observation), mean their float mean, NaN where
    // n is 0.  updateElevationMap resamples the last frame's elevation image on the grid (x0, y0, cell, nx, ny) at every map cell's
    // centre under the map-from-frame pose {a, b, tx, c, d, ty}, adds z_offset (the height of the frame's origin in the map's frame)
    // and updates; (shift_x, shift_y) roll the map first as in updateObstacleMap.
    struct FusedElevationMap {
        double x0 = 0.0, y0 = 0.0, cell = 0.0;  // the map's grid: cell (jx, jy) covers x0 + [jx, jx + 1) * cell, ...
        int nx = 0, ny = 0;
        int n_max = 16;            // 1 .. 1023
        std::vector<int32_t> sum;  // ny x nx, row-major; sized and zeroed by the first update
        std::vector<int16_t> n;    // same shape
        std::vector<float> mean;   // same shape
    };
    void updateElevationMap(FusedElevationMap &map, const double pose[6], double z_offset, double x0, double y0, double cell, int nx, int ny,
                            bool ground_only = false, int shift_x = 0, int shift_y = 0) {
        const pwpp_ground_grid g = {x0, y0, cell, nx, ny, ground_only ? (int32_t)PWPP_GRID_GROUND_ONLY : 0, 0};
        const double mx0 = map.x0 + (double)shift_x * map.cell, my0 = map.y0 + (double)shift_y * map.cell;
        const pwpp_height_map m = {mx0, my0, map.cell, map.nx, map.ny, map.n_max, 0};
        const size_t cells = (size_t)(map.nx > 0 ? map.nx : 0) * (size_t)(map.ny > 0 ? map.ny : 0);
        if (map.sum.size() != cells || map.n.size() != cells) map.sum.assign(cells, 0), map.n.assign(cells, 0);
        std::vector<int32_t> sum(cells ? cells : 1);
        std::vector<int16_t> n(cells ? cells : 1);
        std::vector<float> mean(cells ? cells : 1);
        const int32_t shift[2] = {shift_x, shift_y};
        check(pwpp_fuse_ground(h_, &g, 0, 1, PWPP_MEM_HOST, pose, &z_offset, 1, nullptr, &m, 1, shift, cells ? map.sum.data() : nullptr,
                               cells ? map.n.data() : nullptr, sum.data(), n.data(), mean.data(), nullptr));
        sum.resize(cells), n.resize(cells), mean.resize(cells);
        map.sum.swap(sum), map.n.swap(n), map.mean.swap(mean);
        map.x0 = mx0, map.y0 = my0;
    }
    // (the mean image of such a map, ny x nx: NaN where it was never updated or a cell remembers nothing)
    static Points fusedElevationRows(const FusedElevationMap &map) {
        Points img(map.ny > 0 ? map.ny : 0, map.nx > 0 ? map.nx : 0);
        const size_t cells = (size_t)img.rows() * (size_t)img.cols();
        for (size_t i = 0; i < cells; ++i) img.data()[i] = map.mean.size() == cells ? map.mean[i] : std::numeric_limits<float>::quiet_NaN();
        return img;
    }
    // ... and whether a vehicle can stand or drive on that ground (pwpp_terrain_ground, pwpp_terrain_grid): per cell the height step,
    // the slope (rise over run) and the roughness (metres) of the (2 radius + 1)^2 window around it, NaN where undefined, the number
    // of known cells in the window, and a traversability cost: -1 (none: the cell or its plane is unknown, or fewer than min_known
    // cells), else 0 .. 100, the largest of step / step_max, slope / slope_max and rough / rough_max in per cent, capped.
    struct TerrainParams {
        int radius, min_known;                 // 1 .. 4; 1 .. (2 radius + 1)^2
        float step_max, slope_max, rough_max;  // an infinite limit: that test is off
        TerrainParams()  // (a constructor, not member initialisers: the class is a default argument of its enclosing class's members)
            : radius(1), min_known(3), step_max(std::numeric_limits<float>::infinity()), slope_max(std::numeric_limits<float>::infinity()),
              rough_max(std::numeric_limits<float>::infinity()) {}
    };
    struct Terrain {
        int nx = 0, ny = 0;
        std::vector<float> step, slope, rough;  // ny x nx, row-major: row iy, column ix
        std::vector<uint8_t> count;             // same shape
        std::vector<int8_t> cost;               // same shape
    };
    // (on the last frame's elevation image over the grid (x0, y0, cell, nx, ny))
    Terrain getTerrain(double x0, double y0, double cell, int nx, int ny, const TerrainParams &params = TerrainParams(), bool ground_only = false) {
        const pwpp_ground_grid g = {x0, y0, cell, nx, ny, ground_only ? (int32_t)PWPP_GRID_GROUND_ONLY : 0, 0};
        const pwpp_terrain_params p = {params.radius, params.min_known, params.step_max, params.slope_max, params.rough_max, 0};
        Terrain t = terrain_images(nx, ny);
        check(pwpp_terrain_ground(h_, &g, 0, 1, PWPP_MEM_HOST, &p, t.step.data(), t.slope.data(), t.rough.data(), t.count.data(), t.cost.data(), nullptr));
        return terrain_sized(t);
    }
    // (on the mean of a fused elevation map)
    Terrain fusedTerrain(const FusedElevationMap &map, const TerrainParams &params = TerrainParams()) {
        const pwpp_terrain_params p = {params.radius, params.min_known, params.step_max, params.slope_max, params.rough_max, 0};
        Terrain t = terrain_images(map.nx, map.ny);
        if (map.mean.size() != (size_t)t.nx * (size_t)t.ny || map.mean.empty()) throw std::invalid_argument("fusedTerrain: the map has no mean image of ny x nx cells");
        check(pwpp_terrain_grid(h_, map.nx, map.ny, 1, map.cell, PWPP_MEM_HOST, map.mean.data(), &p, t.step.data(), t.slope.data(), t.rough.data(),
                                t.count.data(), t.cost.data()));
        return terrain_sized(t);
    }
    // ... and what it costs to get there from where the vehicle stands (pwpp_reach_ground, pwpp_reach_grid): per cell the cheapest sum of
    // steps from the source's cell over the 8-connected passable cells of the terrain cost -- a step from a to b costs 5 (across an
    // edge) or 7 (across a corner) times (base + cost(a)) + (base + cost(b)), corners are never cut -- PWPP_REACH_NONE where there is
    // no path, and the index iy * nx + ix of the neighbour the cheapest path comes through (the source: its own; -1: none).
    // reach / (10 base) * cell is a path length in metres on free ground.
    struct ReachParams {
        int base, lethal, unknown, clearance2, max_reach;  // 1 .. 255; 1 .. 101; -1 (impassable) .. 100; >= 0, unused here: no dist2; 0: unlimited
        ReachParams() : base(1), lethal(100), unknown(-1), clearance2(0), max_reach(0) {}  // (a constructor: as TerrainParams)
    };
    struct Reach {
        int nx = 0, ny = 0;
        std::vector<int32_t> reach, from;  // ny x nx, row-major: row iy, column ix
    };
    // (on the terrain cost of the last frame's elevation image over the grid (x0, y0, cell, nx, ny); the source in metres)
    Reach getReach(double x0, double y0, double cell, int nx, int ny, const TerrainParams &terrain_params = TerrainParams(),
                   const ReachParams &reach_params = ReachParams(), double source_x = 0.0, double source_y = 0.0, bool ground_only = false) {
        const pwpp_ground_grid g = {x0, y0, cell, nx, ny, ground_only ? (int32_t)PWPP_GRID_GROUND_ONLY : 0, 0};
        const pwpp_terrain_params tp = {terrain_params.radius, terrain_params.min_known, terrain_params.step_max, terrain_params.slope_max, terrain_params.rough_max, 0};
        const pwpp_reach_params rp = {reach_params.base, reach_params.lethal, reach_params.unknown, reach_params.clearance2, reach_params.max_reach, 0};
        const double source[2] = {source_x, source_y};
        Reach r = reach_images(nx, ny);
        check(pwpp_reach_ground(h_, &g, 0, 1, PWPP_MEM_HOST, &tp, &rp, source, 1, r.reach.data(), r.from.data(), nullptr));
        return reach_sized(r);
    }
    // (on the terrain cost of the mean of a fused elevation map; the source in metres in the map's frame)
    Reach fusedReach(const FusedElevationMap &map, const TerrainParams &terrain_params = TerrainParams(), const ReachParams &reach_params = ReachParams(),
                     double source_x = 0.0, double source_y = 0.0) {
        const pwpp_terrain_params tp = {terrain_params.radius, terrain_params.min_known, terrain_params.step_max, terrain_params.slope_max, terrain_params.rough_max, 0};
        const pwpp_reach_params rp = {reach_params.base, reach_params.lethal, reach_params.unknown, reach_params.clearance2, reach_params.max_reach, 0};
        Reach r = reach_images(map.nx, map.ny);
        const size_t cells = (size_t)r.nx * (size_t)r.ny;
        if (map.mean.size() != cells || map.mean.empty()) throw std::invalid_argument("fusedReach: the map has no mean image of ny x nx cells");
        const pwpp_ground_grid g = {map.x0, map.y0, map.cell, map.nx, map.ny, 0, 0};
        int32_t source[2] = {0, 0};
        check(pwpp_grid_cell_of(&g, source_x, source_y, &source[0], &source[1]));  // (the raster's cell rule; the library names a position it refuses)
        std::vector<int8_t> cost(cells);
        check(pwpp_terrain_grid(h_, map.nx, map.ny, 1, map.cell, PWPP_MEM_HOST, map.mean.data(), &tp, nullptr, nullptr, nullptr, nullptr, cost.data()));
        check(pwpp_reach_grid(h_, map.nx, map.ny, 1, PWPP_MEM_HOST, cost.data(), nullptr, &rp, source, 1, r.reach.data(), r.from.data()));
        return reach_sized(r);
    }
    // ... and the one cost image a planner takes (pwpp_costmap_obstacles, pwpp_costmap_grid): per cell the largest of the occupancy byte's
    // value (occupied 100, free 0), the inflation curve[dist2] to the nearest obstacle -- a table of bytes 0 .. 100 indexed by the
    // squared distance in cells, at most PWPP_COSTMAP_MAX_CURVE entries (inflationCurve builds a common one) -- and the terrain's cost
    // byte; -1 where an enabled layer is unknown and the largest known value is below unknown_below.  why: bits 1, 2, 4 for the
    // layers that set the cost, 8 where a layer stayed unknown.  The image is what getReach's field would be computed on.
    struct CostmapParams {
        int layers;                                               // a mask of PWPP_COSTMAP_OCCUPANCY, _INFLATION, _TERRAIN
        int occupancy_unknown, terrain_unknown, unknown_below;    // -1 (stays unknown) .. 100, twice; 1 .. 101
        CostmapParams() : layers(7), occupancy_unknown(-1), terrain_unknown(-1), unknown_below(101) {}  // (a constructor: as TerrainParams)
    };
    struct Costmap {
        int nx = 0, ny = 0;
        std::vector<int8_t> cost;  // ny x nx, row-major: row iy, column ix
        std::vector<uint8_t> why;  // same shape
    };
    // (the table of pwpp_costmap_curve: 100 up to `inscribed` metres, then floor(peak * exp(-decay * (distance - inscribed))) up to `radius`)
    static std::vector<uint8_t> inflationCurve(double cell, double inscribed, double radius, double decay, int peak = 99) {
        std::vector<uint8_t> curve(PWPP_COSTMAP_MAX_CURVE);
        const int n = pwpp_costmap_curve(cell, inscribed, radius, decay, peak, curve.data(), (int)curve.size());
        check(n);
        curve.resize((size_t)n);
        return curve;
    }
    // (on the last frame over the grid (x0, y0, cell, nx, ny): its visibility bytes, obstacle distances and terrain cost, as the layers ask)
    Costmap getCostmap(double x0, double y0, double cell, int nx, int ny, float h_min, float h_max, const std::vector<uint8_t> &curve,
                       const CostmapParams &params = CostmapParams(), const TerrainParams &terrain_params = TerrainParams(), int min_count = 1,
                       int max_range = 0, double origin_x = 0.0, double origin_y = 0.0, bool ground_only = false) {
        const pwpp_ground_grid g = {x0, y0, cell, nx, ny, ground_only ? (int32_t)PWPP_GRID_GROUND_ONLY : 0, 0};
        const pwpp_terrain_params tp = {terrain_params.radius, terrain_params.min_known, terrain_params.step_max, terrain_params.slope_max, terrain_params.rough_max, 0};
        const pwpp_costmap_params cp = {params.layers, params.occupancy_unknown, params.terrain_unknown, params.unknown_below, {0, 0}};
        const double origin[2] = {origin_x, origin_y};
        Costmap c = costmap_images(nx, ny);
        check(pwpp_costmap_obstacles(h_, &g, h_min, h_max, min_count, origin, 1, max_range, &tp, &cp, curve.empty() ? nullptr : curve.data(), (int)curve.size(), 0, 1,
                                     PWPP_MEM_HOST, c.cost.data(), c.why.data(), nullptr, nullptr, nullptr));
        return costmap_sized(c);
    }
    // (on a fused obstacle map's bytes -- the distances are computed from them on the device -- and, where given, the terrain cost of
    // the mean of a fused elevation map on the SAME grid)
    Costmap fusedCostmap(const FusedObstacleMap &map, const FusedElevationMap *elevation, const std::vector<uint8_t> &curve,
                         const CostmapParams &params = CostmapParams(), const TerrainParams &terrain_params = TerrainParams()) {
        const pwpp_terrain_params tp = {terrain_params.radius, terrain_params.min_known, terrain_params.step_max, terrain_params.slope_max, terrain_params.rough_max, 0};
        const pwpp_costmap_params cp = {params.layers, params.occupancy_unknown, params.terrain_unknown, params.unknown_below, {0, 0}};
        Costmap c = costmap_images(map.nx, map.ny);
        const size_t cells = (size_t)c.nx * (size_t)c.ny;
        if (map.occupancy.size() != cells || map.occupancy.empty()) throw std::invalid_argument("fusedCostmap: the map has no occupancy image of ny x nx cells");
        std::vector<int8_t> terrain;
        if (elevation) {
            if (elevation->x0 != map.x0 || elevation->y0 != map.y0 || elevation->cell != map.cell || elevation->nx != map.nx || elevation->ny != map.ny)
                throw std::invalid_argument("fusedCostmap: the elevation map's grid is not the obstacle map's");
            if (elevation->mean.size() != cells) throw std::invalid_argument("fusedCostmap: the elevation map has no mean image of ny x nx cells");
            terrain.resize(cells);
            check(pwpp_terrain_grid(h_, map.nx, map.ny, 1, map.cell, PWPP_MEM_HOST, elevation->mean.data(), &tp, nullptr, nullptr, nullptr, nullptr, terrain.data()));
        }
        check(pwpp_costmap_grid(h_, map.nx, map.ny, 1, PWPP_MEM_HOST, map.occupancy.data(), elevation ? terrain.data() : nullptr, nullptr, &cp,
                                curve.empty() ? nullptr : curve.data(), (int)curve.size(), c.cost.data(), c.why.data()));
        return costmap_sized(c);
    }
    // ... and the way itself (pwpp_plan_grid): for every start position the chain of `from` of the reach field from the start's cell to the
    // source's, one row of sums per route (status PWPP_ROUTE_OK / _NONE / _BROKEN, cells, cost == reach[start], edge and corner steps --
    // length = cell * (edge_steps + sqrt(2) corner_steps) -- the largest term, waypoints), the cells, and the waypoints a controller
    // tracks: greedy shortcuts of at most `look` cells whose line crosses only cells with a term <= base + line_cost and cuts no corner.
    // Lists run from the start to the source (step costs are symmetric: put the source at the goal); -1 / NaN behind a list's end.
    struct RouteParams {
        int max_cells, max_waypoints, look, line_cost;  // >= 0, twice (0: no list); 1 .. 256; 0 .. 100
        RouteParams() : max_cells(1024), max_waypoints(64), look(64), line_cost(0) {}  // (a constructor: as TerrainParams)
    };
    struct Routes {
        int n = 0, max_cells = 0, max_waypoints = 0;
        std::vector<pwpp_route> rows;           // n
        std::vector<int32_t> cells, waypoints;  // n x max_cells, n x max_waypoints: cell indices iy * nx + ix
        std::vector<double> waypoints_xy;       // n x max_waypoints x {x, y}: the centres of those cells in metres
    };
    // (on the terrain cost of the last frame's elevation image over the grid (x0, y0, cell, nx, ny); starts_xy: n x {x, y} in metres, the source in metres)
    Routes getRoutes(double x0, double y0, double cell, int nx, int ny, const std::vector<double> &starts_xy, const TerrainParams &terrain_params = TerrainParams(),
                     const ReachParams &reach_params = ReachParams(), const RouteParams &route_params = RouteParams(), double source_x = 0.0, double source_y = 0.0,
                     bool ground_only = false) {
        const pwpp_ground_grid g = {x0, y0, cell, nx, ny, ground_only ? (int32_t)PWPP_GRID_GROUND_ONLY : 0, 0};
        const pwpp_terrain_params tp = {terrain_params.radius, terrain_params.min_known, terrain_params.step_max, terrain_params.slope_max, terrain_params.rough_max, 0};
        const size_t cells = (size_t)(nx > 0 ? nx : 0) * (size_t)(ny > 0 ? ny : 0);
        std::vector<int8_t> cost(cells ? cells : 1);  // (room for one cell where the grid has none: the library names the grid)
        check(pwpp_terrain_ground(h_, &g, 0, 1, PWPP_MEM_HOST, &tp, nullptr, nullptr, nullptr, nullptr, cost.data(), nullptr));
        cost.resize(cells);
        return planRoutes(cost, x0, y0, cell, nx, ny, starts_xy, reach_params, route_params, source_x, source_y);
    }
    // (on any cost image of ny x nx cells over that grid -- a Costmap's cost)
    Routes planRoutes(const std::vector<int8_t> &cost, double x0, double y0, double cell, int nx, int ny, const std::vector<double> &starts_xy,
                      const ReachParams &reach_params = ReachParams(), const RouteParams &route_params = RouteParams(), double source_x = 0.0, double source_y = 0.0) {
        const pwpp_ground_grid g = {x0, y0, cell, nx, ny, 0, 0};
        const pwpp_reach_params rp = {reach_params.base, reach_params.lethal, reach_params.unknown, reach_params.clearance2, reach_params.max_reach, 0};
        const pwpp_route_params qp = {route_params.max_cells, route_params.max_waypoints, route_params.look, route_params.line_cost};
        if (starts_xy.empty() || starts_xy.size() % 2 != 0) throw std::invalid_argument("planRoutes: starts_xy holds n x {x, y}, n >= 1");
        if (nx < 1 || ny < 1 || cost.size() != (size_t)nx * (size_t)ny) throw std::invalid_argument("planRoutes: the cost image has not ny x nx cells");
        Routes r;
        r.n = (int)(starts_xy.size() / 2), r.max_cells = qp.max_cells > 0 ? qp.max_cells : 0, r.max_waypoints = qp.max_waypoints > 0 ? qp.max_waypoints : 0;
        int32_t source[2] = {0, 0};
        check(pwpp_grid_cell_of(&g, source_x, source_y, &source[0], &source[1]));  // (the raster's cell rule; the library names a position it refuses)
        std::vector<int32_t> start(starts_xy.size());
        for (int i = 0; i < r.n; ++i) check(pwpp_grid_cell_of(&g, starts_xy[2 * (size_t)i], starts_xy[2 * (size_t)i + 1], &start[2 * (size_t)i], &start[2 * (size_t)i + 1]));
        r.rows.resize((size_t)r.n), r.cells.assign((size_t)r.n * (size_t)r.max_cells, -1), r.waypoints.assign((size_t)r.n * (size_t)r.max_waypoints, -1);
        check(pwpp_plan_grid(h_, nx, ny, 1, PWPP_MEM_HOST, cost.data(), nullptr, &rp, source, 1, start.data(), 1, r.n, &qp, r.rows.data(),
                             r.max_cells ? r.cells.data() : nullptr, r.max_waypoints ? r.waypoints.data() : nullptr, nullptr, nullptr));
        r.waypoints_xy.assign(2 * r.waypoints.size(), std::numeric_limits<double>::quiet_NaN());
        for (size_t i = 0; i < r.waypoints.size(); ++i)
            if (r.waypoints[i] >= 0) {
                r.waypoints_xy[2 * i] = x0 + ((double)(r.waypoints[i] % nx) + 0.5) * cell;
                r.waypoints_xy[2 * i + 1] = y0 + ((double)(r.waypoints[i] / nx) + 0.5) * cell;
            }
        return r;
    }
    // ... and whether the vehicle fits along the way (pwpp_footprint_grid): a fan of candidate trajectories, n_traj x n_steps poses {x, y, yaw}
    // in metres and radians, the rectangle [-rear, front] x [-half_width, half_width] metres round each pose laid over the cost image and
    // judged cell by cell with the reach's rule.  Per pose a row (status PWPP_FOOT_FREE / _HIT / _SKIPPED, the cells covered, outside the
    // image, blocked and unknown, the dearest term, the first blocked cell), per trajectory the first pose that hits and the sums over
    // the free poses before it; reach_last where a reach field is given.  A pose whose yaw is NaN is skipped: how ragged fans are padded.
    // pad > 0 widens the rectangle by so many ticks of 1/16 cell on every side: 12 covers every cell the rectangle touches at all.
    struct FootprintParams {
        double front, rear, half_width;  // metres; each at most 64 cells
        int pad;                         // ticks of 1/16 cell added on every side, >= 0
        bool outside_blocks;             // a covered cell outside the image makes the pose a hit
        FootprintParams() : front(3.4), rear(1.1), half_width(0.9), pad(0), outside_blocks(false) {}  // (a constructor: as TerrainParams)
    };
    struct Footprints {
        int n_traj = 0, n_steps = 0;
        std::vector<pwpp_footprint_pose_row> poses;         // n_traj x n_steps
        std::vector<pwpp_footprint_traj_row> trajectories;  // n_traj
    };
    // (on any cost image of ny x nx cells over the grid (x0, y0, cell, nx, ny) -- a Costmap's cost; poses_xyyaw: n_traj x n_steps x {x, y, yaw}; reach: empty or a Reach's field)
    Footprints checkFootprints(const std::vector<int8_t> &cost, double x0, double y0, double cell, int nx, int ny, const std::vector<double> &poses_xyyaw, int n_steps,
                               const FootprintParams &footprint_params = FootprintParams(), const ReachParams &reach_params = ReachParams(),
                               const std::vector<int32_t> &reach = std::vector<int32_t>()) {
        const pwpp_ground_grid g = {x0, y0, cell, nx, ny, 0, 0};
        const pwpp_reach_params rp = {reach_params.base, reach_params.lethal, reach_params.unknown, reach_params.clearance2, reach_params.max_reach, 0};
        if (n_steps < 1 || poses_xyyaw.empty() || poses_xyyaw.size() % (3 * (size_t)n_steps) != 0)
            throw std::invalid_argument("checkFootprints: poses_xyyaw holds n_traj x n_steps x {x, y, yaw}, n_traj >= 1");
        if (nx < 1 || ny < 1 || cost.size() != (size_t)nx * (size_t)ny) throw std::invalid_argument("checkFootprints: the cost image has not ny x nx cells");
        if (!reach.empty() && reach.size() != cost.size()) throw std::invalid_argument("checkFootprints: the reach field has not the cost image's cells");
        if (!(cell > 0.0) || footprint_params.pad < 0) throw std::invalid_argument("checkFootprints: a positive cell and a pad >= 0 expected");
        const double ticks = PWPP_FOOT_SUB / cell;
        const auto extent = [&](double metres) { return metres >= 0.0 && metres * ticks <= 2.0 * PWPP_FOOT_MAX_EXTENT ? (int32_t)std::lround(metres * ticks) + footprint_params.pad : (int32_t)-1; };
        const pwpp_footprint_params fp = {extent(footprint_params.front), extent(footprint_params.rear), extent(footprint_params.half_width),
                                          footprint_params.outside_blocks ? (int32_t)PWPP_FOOT_OUTSIDE_BLOCKS : 0, {0, 0}};  // (the library names an extent it refuses)
        Footprints r;
        r.n_steps = n_steps, r.n_traj = (int)(poses_xyyaw.size() / (3 * (size_t)n_steps));
        std::vector<int32_t> poses(4 * (size_t)r.n_traj * (size_t)n_steps, 0);
        for (size_t i = 0; i < poses.size() / 4; ++i)
            if (!std::isnan(poses_xyyaw[3 * i + 2])) check(pwpp_footprint_pose(&g, poses_xyyaw[3 * i], poses_xyyaw[3 * i + 1], poses_xyyaw[3 * i + 2], &poses[4 * i]));
        r.poses.resize((size_t)r.n_traj * (size_t)n_steps), r.trajectories.resize((size_t)r.n_traj);
        check(pwpp_footprint_grid(h_, nx, ny, 1, PWPP_MEM_HOST, cost.data(), nullptr, reach.empty() ? nullptr : reach.data(), &rp, &fp, poses.data(), 1, r.n_traj, n_steps,
                                  r.poses.data(), r.trajectories.data()));
        return r;
    }
    // ... and where the last frame fits that map (pwpp_match_obstacles): for every candidate pose (n_candidates x {a, b, tx, c, d, ty},
    // the prior first) and every shift of [-wx, wx] x [-wy, wy] map cells, the sum of log_odds under the occupied cells of the
    // frame's visibility bytes; the best by the contract's order, and `pose`, the winning candidate moved by the winning shift
    // (pwpp_match_pose): what updateObstacleMap takes next.  The map is read, not changed; it must have been updated once.
    struct ObstacleMatch {
        int candidate = -1, sx = 0, sy = 0;
        int64_t score = 0;
        int cells = 0;  // occupied cells of the frame
        double pose[6] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    };
    ObstacleMatch matchObstacleMap(const FusedObstacleMap &map, const double *candidates, int n_candidates, int wx, int wy, double x0, double y0,
                                   double cell, int nx, int ny, float h_min, float h_max, int min_count = 1, int max_range = 0, double origin_x = 0.0,
                                   double origin_y = 0.0) {
        const pwpp_ground_grid g = {x0, y0, cell, nx, ny, 0, 0};
        const pwpp_fusion_map m = {map.x0, map.y0, map.cell, map.nx, map.ny, map.hit, map.miss, map.l_min, map.l_max, map.occupied_at, map.free_at};
        const size_t cells = (size_t)(map.nx > 0 ? map.nx : 0) * (size_t)(map.ny > 0 ? map.ny : 0);
        if (map.log_odds.size() != cells || cells == 0) throw std::runtime_error("matchObstacleMap: the map has no log_odds of its nx x ny cells");
        const double origin[2] = {origin_x, origin_y};
        pwpp_match_best best = {0, -1, 0, 0, 0};
        check(pwpp_match_obstacles(h_, &g, h_min, h_max, min_count, origin, 1, max_range, 0, 1, PWPP_MEM_HOST, candidates, 1, n_candidates, nullptr, &m, 1,
                                   map.log_odds.data(), wx, wy, &best, nullptr, nullptr));
        ObstacleMatch r;
        r.candidate = best.candidate, r.sx = best.sx, r.sy = best.sy, r.score = best.score, r.cells = best.cells;
        if (best.candidate >= 0 && best.candidate < n_candidates) check(pwpp_match_pose(candidates + 6 * (size_t)best.candidate, map.cell, best.sx, best.sy, r.pose));
        return r;
    }
    // ... and every cluster as an oriented box (pwpp_box_obstacles on the labels above): centre, heading, length and width in
    // metres, the spread along and across, the extent in height over ground and in z.  boxes[r] belongs to clusters[r].
    struct ObstacleBoxes {
        std::vector<int32_t> label;                   // ny x nx, row-major
        std::vector<pwpp_obstacle_cluster> clusters;  // one row per cluster
        std::vector<pwpp_obstacle_box> boxes;         // one box per cluster
        int count = 0;                                // clusters.size() == boxes.size()
    };
    ObstacleBoxes getObstacleBoxes(double x0, double y0, double cell, int nx, int ny, float h_min, float h_max, int min_count = 1, int connectivity = 8,
                                   bool ground_only = false) {
        ObstacleClusters c = getObstacleClusters(x0, y0, cell, nx, ny, h_min, h_max, min_count, connectivity, ground_only);
        ObstacleBoxes b;
        b.count = c.count;
        if (c.count > 0) {
            const pwpp_ground_grid g = {x0, y0, cell, nx, ny, ground_only ? (int32_t)PWPP_GRID_GROUND_ONLY : 0, 0};
            b.boxes.resize((size_t)c.count);
            check(pwpp_box_obstacles(h_, &g, h_min, h_max, 0, 1, PWPP_MEM_HOST, c.label.data(), b.boxes.data(), c.count));
        }
        b.label = std::move(c.label);
        b.clusters = std::move(c.clusters);
        return b;
    }
    // ... and every cluster's outline (pwpp_hull_obstacles on the labels above): the convex hull of its points on the grid's 1/1024 m
    // lattice and the enclosing rectangle of least area -- centre, unit vector of the side it stands on, length and width in metres.
    // hulls[r] belongs to clusters[r]; vertices holds max_vertices {qx, qy} pairs per row, the first hulls[r].stored written
    // (vertexXY gives one in metres).  A hull of more than max_vertices vertices has its true count, its area and no rectangle.
    struct ObstacleHulls {
        std::vector<int32_t> label;                   // ny x nx, row-major
        std::vector<pwpp_obstacle_cluster> clusters;  // one row per cluster
        std::vector<pwpp_obstacle_hull> hulls;        // one row per cluster
        std::vector<int32_t> vertices;                // count x max_vertices x 2
        int count = 0, max_vertices = 0;
        double x0 = 0.0, y0 = 0.0;
        void vertexXY(int row, int k, double &x, double &y) const {
            const int32_t *q = &vertices[((size_t)row * (size_t)max_vertices + (size_t)k) * 2];
            x = (double)(x0 + (double)q[0] / 1024.0), y = (double)(y0 + (double)q[1] / 1024.0);
        }
    };
    ObstacleHulls getObstacleHulls(double x0, double y0, double cell, int nx, int ny, float h_min, float h_max, int max_vertices = 32, int min_count = 1,
                                   int connectivity = 8, bool ground_only = false) {
        ObstacleClusters c = getObstacleClusters(x0, y0, cell, nx, ny, h_min, h_max, min_count, connectivity, ground_only);
        ObstacleHulls o;
        o.count = c.count, o.max_vertices = max_vertices, o.x0 = x0, o.y0 = y0;
        if (c.count > 0) {
            const pwpp_ground_grid g = {x0, y0, cell, nx, ny, ground_only ? (int32_t)PWPP_GRID_GROUND_ONLY : 0, 0};
            o.hulls.resize((size_t)c.count);
            o.vertices.assign((size_t)c.count * (size_t)(max_vertices > 0 ? max_vertices : 0) * 2, 0);
            check(pwpp_hull_obstacles(h_, &g, h_min, h_max, 0, 1, PWPP_MEM_HOST, c.label.data(), o.hulls.data(), c.count, o.vertices.empty() ? nullptr : o.vertices.data(),
                                      max_vertices));
        }
        o.label = std::move(c.label);
        o.clusters = std::move(c.clusters);
        return o;
    }
    // ... and which cluster is which cluster of the call before (pwpp_track_obstacles): the labelling as getObstacleClusters gives it,
    // associated with the label image this object kept from its previous call on a grid of the same sides, under the pose {a, b, tx,
    // c, d, ty} that says where a position of the previous frame lies in this one (the identity: null).  ids[r] is the persistent
    // id of cluster r: a cluster that is the mutual best partner of one of the previous call's, sharing at least min_overlap cells,
    // keeps that one's id, every other one gets the next unused id; curr_links[r] and prev_links[r] are the rows of include/pwpp.h
    // (links > 1: a merge, on the previous side a split).  At most max_clusters clusters are tracked; the cells of further ones
    // count as unlabelled.  The object keeps the label image, the ids and the next id between calls -- the library's handle keeps
    // nothing -- until resetObstacleTracks(), or a call with other sides or another max_clusters, which starts afresh.
    struct ObstacleTracks {
        int nx = 0, ny = 0;
        std::vector<int32_t> label;                   // ny x nx, row-major: row iy, column ix
        std::vector<pwpp_obstacle_cluster> clusters;  // min(count, max_clusters) rows
        std::vector<pwpp_cluster_link> curr_links;    // one per row of clusters
        std::vector<pwpp_cluster_link> prev_links;    // max_clusters rows: the previous call's clusters
        std::vector<int32_t> ids;                     // one per row of clusters
        int count = 0;                                // the true number of clusters
        int pairs = 0;                                // the number of (previous, current) pairs sharing a cell; max_pairs + 1: too many, no links
    };
    ObstacleTracks trackObstacleClusters(double x0, double y0, double cell, int nx, int ny, float h_min, float h_max, const double *pose = nullptr,
                                         int min_count = 1, int connectivity = 8, int max_clusters = 256, int gate = 1, int min_overlap = 1) {
        const pwpp_ground_grid g = {x0, y0, cell, nx, ny, 0, 0};
        const double identity[6] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0};
        ObstacleTracks t;
        t.nx = nx > 0 ? nx : 0, t.ny = ny > 0 ? ny : 0;
        const size_t cells = (size_t)t.nx * (size_t)t.ny, rows = (size_t)(max_clusters > 0 ? max_clusters : 0);
        if (track_label_.size() != cells || track_ids_.size() != rows || track_nx_ != t.nx) resetObstacleTracks();
        if (track_label_.empty()) track_label_.assign(cells ? cells : 1, -1), track_ids_.assign(rows ? rows : 1, -1), track_nx_ = t.nx;
        t.label.assign(cells ? cells : 1, -1), t.clusters.resize(rows ? rows : 1), t.curr_links.resize(rows ? rows : 1), t.prev_links.resize(rows ? rows : 1);
        t.ids.assign(rows ? rows : 1, -1);
        int32_t n = 0, pairs = 0, next = track_next_id_;
        const int max_pairs = max_clusters > 0 && max_clusters <= (1 << 22) ? 4 * max_clusters : 1 << 24;
        check(pwpp_track_obstacles(h_, &g, h_min, h_max, min_count, connectivity, 0, 1, PWPP_MEM_HOST, t.label.data(), nullptr, nullptr, t.clusters.data(), &n,
                                   max_clusters, nullptr, track_label_.data(), pose ? pose : identity, 1, gate, min_overlap, max_pairs, t.curr_links.data(),
                                   t.prev_links.data(), &pairs, track_ids_.data(), &track_next_id_, t.ids.data(), &next));
        track_label_ = t.label, track_ids_ = t.ids, track_next_id_ = next;
        t.count = n, t.pairs = pairs;
        const size_t kept = (size_t)(n < max_clusters ? n : max_clusters);
        t.label.resize(cells), t.clusters.resize(kept), t.curr_links.resize(kept), t.ids.resize(kept), t.prev_links.resize(rows);
        return t;
    }
    void resetObstacleTracks() {
        track_label_.clear(), track_ids_.clear();
        track_next_id_ = 0, track_nx_ = 0;
    }
    // ... and what a fused obstacle map holds under every cluster (pwpp_evidence_obstacles): the labelling as getObstacleClusters
    // gives it, and per cluster the cells that land in the map under the pose {a, b, tx, c, d, ty} (map-from-frame, the pose of
    // updateObstacleMap; the identity: null), counted by the class of the map's largest log-odds within `gate` cells, and the
    // verdict -- PWPP_EVID_MOVING: at least moving_share / 256 of the landed cells read free; PWPP_EVID_STATIC: at least
    // static_share / 256 read occupied; PWPP_EVID_UNDECIDED -- rows[r] belongs to clusters[r] and, by the same row, to ids[r] of
    // trackObstacleClusters.  With `occupancy` (ny x nx bytes, those of getObstacleVisibility) `masked` is those bytes with the
    // cells of moving clusters set to PWPP_OCC_UNKNOWN: what pwpp_fuse_grid takes so that the map is fused without its movers.
    // The map is read, not changed; it must have been updated once.
    struct EvidenceRule {
        int gate, min_cells, moving_share, static_share;  // 0 .. 4; >= 1; 1 .. 256; 1 .. 256
        EvidenceRule() : gate(1), min_cells(3), moving_share(192), static_share(192) {}  // (a constructor: as TerrainParams)
    };
    struct ObstacleEvidence {
        int nx = 0, ny = 0;
        std::vector<int32_t> label;                   // ny x nx, row-major: row iy, column ix
        std::vector<pwpp_obstacle_cluster> clusters;  // min(count, max_clusters) rows
        std::vector<pwpp_cluster_evidence> rows;      // one per row of clusters
        std::vector<int8_t> cell_class;               // ny x nx: the class byte of a labelled, landed cell, PWPP_EVID_CELL_NONE elsewhere
        std::vector<int8_t> masked;                   // ny x nx with `occupancy`, else empty
        int count = 0;                                // the true number of clusters
    };
    ObstacleEvidence getObstacleEvidence(const FusedObstacleMap &map, double x0, double y0, double cell, int nx, int ny, float h_min, float h_max,
                                         const double *pose = nullptr, const EvidenceRule &rule = EvidenceRule(), const int8_t *occupancy = nullptr,
                                         int min_count = 1, int connectivity = 8, int max_clusters = 256) {
        const pwpp_ground_grid g = {x0, y0, cell, nx, ny, 0, 0};
        const pwpp_fusion_map m = {map.x0, map.y0, map.cell, map.nx, map.ny, map.hit, map.miss, map.l_min, map.l_max, map.occupied_at, map.free_at};
        const pwpp_evidence_rule r = {rule.gate, rule.min_cells, rule.moving_share, rule.static_share};
        const double identity[6] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0};
        const size_t map_cells = (size_t)(map.nx > 0 ? map.nx : 0) * (size_t)(map.ny > 0 ? map.ny : 0);
        if (map.log_odds.size() != map_cells || map_cells == 0) throw std::runtime_error("getObstacleEvidence: the map has no log_odds of its nx x ny cells");
        ObstacleEvidence e;
        e.nx = nx > 0 ? nx : 0, e.ny = ny > 0 ? ny : 0;
        const size_t cells = (size_t)e.nx * (size_t)e.ny, rows = (size_t)(max_clusters > 0 ? max_clusters : 0);
        e.label.assign(cells ? cells : 1, -1), e.clusters.resize(rows ? rows : 1), e.rows.resize(rows ? rows : 1), e.cell_class.resize(cells ? cells : 1);
        if (occupancy) e.masked.resize(cells ? cells : 1);
        int32_t n = 0;
        check(pwpp_evidence_obstacles(h_, &g, h_min, h_max, min_count, connectivity, 0, 1, PWPP_MEM_HOST, e.label.data(), nullptr, nullptr, e.clusters.data(), &n,
                                      max_clusters, nullptr, occupancy, pose ? pose : identity, 1, nullptr, &m, 1, map.log_odds.data(), &r, e.rows.data(),
                                      e.cell_class.data(), occupancy ? e.masked.data() : nullptr));
        e.count = n;
        const size_t kept = (size_t)(n < max_clusters ? n : max_clusters);
        e.label.resize(cells), e.cell_class.resize(cells), e.clusters.resize(kept), e.rows.resize(kept);
        if (occupancy) e.masked.resize(cells);
        return e;
    }
#ifdef PWPP_HAVE_EIGEN
    std::vector<pwpp_ground_sample> queryGround(const Eigen::MatrixX3f &positions) {
        std::vector<float> xyz((size_t)positions.rows() * 3);
        for (int i = 0; i < (int)positions.rows(); ++i)
            for (int j = 0; j < 3; ++j) xyz[(size_t)i * 3 + (size_t)j] = positions(i, j);
        return queryGround(xyz.data(), (int)positions.rows());
    }
    Eigen::MatrixXf getElevationMap(double x0, double y0, double cell, int nx, int ny, bool ground_only = false) {
        return to_eigen(elevationMapRows(x0, y0, cell, nx, ny, ground_only));
    }
    Eigen::MatrixXf getFusedElevation(const FusedElevationMap &map) { return to_eigen(fusedElevationRows(map)); }
#else
    Points getElevationMap(double x0, double y0, double cell, int nx, int ny, bool ground_only = false) {
        return elevationMapRows(x0, y0, cell, nx, ny, ground_only);
    }
    Points getFusedElevation(const FusedElevationMap &map) { return fusedElevationRows(map); }
#endif

#ifdef PWPP_HAVE_EIGEN
    // the reference's return types (fresh objects on every call, as the reference's toEigenCloud / toIndices, :8-26)
    Eigen::MatrixX3f getGround() { return to_eigen(xyz(true)); }               // reference :157
    Eigen::MatrixX3f getNonground() { return to_eigen(xyz(false)); }           // reference :158
    Eigen::VectorXi getGroundIndices() { return to_eigen(idx(true)); }         // reference :159
    Eigen::VectorXi getNongroundIndices() { return to_eigen(idx(false)); }     // reference :160
    Eigen::MatrixX3f getCenters() { return to_eigen(rows(true)); }             // reference :162
    Eigen::MatrixX3f getNormals() { return to_eigen(rows(false)); }            // reference :163
#else
    Cloud getGround() { return xyz(true); }          // reference :157
    Cloud getNonground() { return xyz(false); }      // reference :158
    Indices getGroundIndices() { return idx(true); }      // reference :159
    Indices getNongroundIndices() { return idx(false); }  // reference :160
    Cloud getCenters() { return rows(true); }        // reference :162
    Cloud getNormals() { return rows(false); }       // reference :163
#endif
    // the same results as plain containers, whatever the build (row-major (rows, 3) floats / int32)
    Cloud groundCloud() { return xyz(true); }
    Cloud nongroundCloud() { return xyz(false); }
    Indices groundIndexList() { return idx(true); }
    Indices nongroundIndexList() { return idx(false); }

    pwpp_handle *handle() { return h_; }  // escape hatch to the batch API of include/pwpp.h

private:
    patchwork::Params params_;
    pwpp_handle *h_;
    std::vector<int32_t> track_label_, track_ids_;  // trackObstacleClusters: the previous call's label image and ids
    int32_t track_next_id_ = 0;
    int track_nx_ = 0;

    // (the five images of a terrain call, with room for one cell where the grid has none: the library names the bad argument)
    static Terrain terrain_images(int nx, int ny) {
        Terrain t;
        t.nx = nx > 0 ? nx : 0, t.ny = ny > 0 ? ny : 0;
        const size_t cells = (size_t)t.nx * (size_t)t.ny, room = cells ? cells : 1;
        t.step.assign(room, 0.0f), t.slope.assign(room, 0.0f), t.rough.assign(room, 0.0f), t.count.assign(room, 0), t.cost.assign(room, -1);
        return t;
    }
    static Terrain &terrain_sized(Terrain &t) {
        const size_t cells = (size_t)t.nx * (size_t)t.ny;
        t.step.resize(cells), t.slope.resize(cells), t.rough.resize(cells), t.count.resize(cells), t.cost.resize(cells);
        return t;
    }
    // (the two images of a reach call, with room for one cell where the grid has none, as terrain_images)
    static Reach reach_images(int nx, int ny) {
        Reach r;
        r.nx = nx > 0 ? nx : 0, r.ny = ny > 0 ? ny : 0;
        const size_t cells = (size_t)r.nx * (size_t)r.ny, room = cells ? cells : 1;
        r.reach.assign(room, PWPP_REACH_NONE), r.from.assign(room, -1);
        return r;
    }
    static Reach &reach_sized(Reach &r) {
        const size_t cells = (size_t)r.nx * (size_t)r.ny;
        r.reach.resize(cells), r.from.resize(cells);
        return r;
    }
    // (the two images of a costmap call, with room for one cell where the grid has none, as terrain_images)
    static Costmap costmap_images(int nx, int ny) {
        Costmap c;
        c.nx = nx > 0 ? nx : 0, c.ny = ny > 0 ? ny : 0;
        const size_t cells = (size_t)c.nx * (size_t)c.ny, room = cells ? cells : 1;
        c.cost.assign(room, -1), c.why.assign(room, 0);
        return c;
    }
    static Costmap &costmap_sized(Costmap &c) {
        const size_t cells = (size_t)c.nx * (size_t)c.ny;
        c.cost.resize(cells), c.why.resize(cells);
        return c;
    }
#ifdef PWPP_HAVE_EIGEN
    static Eigen::MatrixX3f to_eigen(const Cloud &c) {
        Eigen::MatrixX3f m(c.rows(), 3);
        for (int i = 0; i < c.rows(); ++i)
            for (int j = 0; j < 3; ++j) m(i, j) = c(i, j);
        return m;
    }
    static Eigen::MatrixXf to_eigen(const Points &c) {
        Eigen::MatrixXf m(c.rows(), c.cols());
        for (int i = 0; i < c.rows(); ++i)
            for (int j = 0; j < c.cols(); ++j) m(i, j) = c(i, j);
        return m;
    }
    static Eigen::VectorXi to_eigen(const Indices &v) {
        Eigen::VectorXi m(v.rows());
        for (int i = 0; i < v.rows(); ++i) m(i) = v(i);
        return m;
    }
#endif
    static void check(int rc) {
        if (rc < 0) throw std::runtime_error(std::string("patchworkpp (HIP): ") + pwpp_last_error());
    }
    // the reference's verbose lines (patchworkpp.cpp:323-335), with GPU times: czm = binning kernels, sort = 0 (this
    // design has no sort), pca = the fit kernels, estimate = GLE / TGR + the index lists
    void report_times() {
        double ms[PWPP_NUM_KERNELS];
        int64_t launches[PWPP_NUM_KERNELS];
        check(pwpp_get_kernel_profile(h_, ms, launches));
        check(pwpp_reset_kernel_profile(h_));
        const double czm = ms[0] + ms[1] + ms[2], pca = ms[3] + ms[4] + ms[5] + ms[6] + ms[7] + ms[8], est = ms[9] + ms[10];
        std::cout << "Time taken : " << pwpp_get_time_us(h_) / 1e6 << "(sec) ~ " << czm / 1e3 << "(czm) + " << 0.0 << "(sort) + "
                  << pca / 1e3 << "(pca) + " << est / 1e3 << "(estimate)" << std::endl;
        std::cout << "\033[1;32m" << "PatchWorkpp::estimateGround() - Estimation is finished !" << "\033[0m" << std::endl;
    }
    void counts(int32_t &g, int32_t &n, int32_t &p) { check(pwpp_get_counts(h_, 0, &g, &n, &p)); }
    Cloud xyz(bool ground) {
        int32_t g, n, p;
        counts(g, n, p);
        Cloud c(ground ? g : n);
        check(ground ? pwpp_get_ground_xyz(h_, 0, c.data()) : pwpp_get_nonground_xyz(h_, 0, c.data()));
        return c;
    }
    Indices idx(bool ground) {
        int32_t g, n, p;
        counts(g, n, p);
        Indices v(ground ? g : n);
        check(ground ? pwpp_get_ground_indices(h_, 0, v.data()) : pwpp_get_nonground_indices(h_, 0, v.data()));
        return v;
    }
    Labels labels() {
        pwpp_device_view v;
        check(pwpp_get_device_view(h_, &v));
        Labels l((int)(v.frame_base[1] - v.frame_base[0]));
        check(pwpp_get_labels(h_, 0, l.data()));
        return l;
    }
    int frame_points() {
        pwpp_device_view v;
        check(pwpp_get_device_view(h_, &v));
        return (int)(v.frame_base[1] - v.frame_base[0]);
    }
    Indices pointPatches() {
        Indices v(frame_points());
        check(pwpp_get_point_patches(h_, 0, v.data()));
        return v;
    }
    Distances pointDistances() {
        Distances v(frame_points());
        check(pwpp_get_point_distances(h_, 0, v.data()));
        return v;
    }
    Points points(bool ground) {  // (the class only takes matrices: a record is a row of `cols` floats)
        int32_t g, n, p;
        counts(g, n, p);
        const int rb = pwpp_get_record_bytes(h_);
        check(rb);
        Points c(ground ? g : n, rb / (int)sizeof(float));
        check(ground ? pwpp_get_ground_records(h_, 0, c.data()) : pwpp_get_nonground_records(h_, 0, c.data()));
        return c;
    }
    Cloud rows(bool centers) {
        int32_t g, n, p;
        counts(g, n, p);
        Cloud c(p);
        check(centers ? pwpp_get_centers(h_, 0, c.data()) : pwpp_get_normals(h_, 0, c.data()));
        return c;
    }
};

}  // namespace patchwork

#endif
