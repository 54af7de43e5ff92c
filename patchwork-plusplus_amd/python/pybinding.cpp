// pybinding.cpp -- Python module `pypatchworkpp` with the reference's API surface
// (/root/reference/python/patchworkpp/pybinding.cpp:9-57: classes `Parameters` and
// `patchworkpp`, same attribute and method names), backed by the MI355X library.
//
// The reference binds Eigen types through pybind11/eigen.h; there is no Eigen here, so
// arrays cross as numpy buffers directly: estimateGround() takes any 2-D array convertible
// to float32 (C- or F-contiguous is used in place, anything else is copied), the getters
// return fresh C-contiguous numpy arrays: (n, 3) float32 and (n,) int32.  The GIL is
// released while the GPU works.
#include <array>

#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "patchwork/patchworkpp.h"

namespace py = pybind11;
using patchwork::Params;
using patchwork::PatchWorkpp;

namespace {

py::array_t<float> to_numpy(const patchwork::Cloud &c) {
    py::array_t<float> out({(py::ssize_t)c.rows(), (py::ssize_t)3});
    if (c.rows() > 0) std::memcpy(out.mutable_data(), c.data(), (size_t)c.rows() * 3 * sizeof(float));
    return out;
}
py::array_t<uint8_t> to_numpy(const patchwork::Labels &v) {
    py::array_t<uint8_t> out((py::ssize_t)v.rows());
    if (v.rows() > 0) std::memcpy(out.mutable_data(), v.data(), (size_t)v.rows());
    return out;
}
py::array_t<float> to_numpy(const patchwork::Distances &v) {
    py::array_t<float> out((py::ssize_t)v.rows());
    if (v.rows() > 0) std::memcpy(out.mutable_data(), v.data(), (size_t)v.rows() * sizeof(float));
    return out;
}
py::array_t<float> to_numpy(const patchwork::Points &v) {
    py::array_t<float> out({(py::ssize_t)v.rows(), (py::ssize_t)v.cols()});
    if (v.rows() > 0) std::memcpy(out.mutable_data(), v.data(), (size_t)v.rows() * (size_t)v.cols() * sizeof(float));
    return out;
}
py::array_t<int32_t> to_numpy(const patchwork::Indices &v) {
    py::array_t<int32_t> out((py::ssize_t)v.rows());
    if (v.rows() > 0) std::memcpy(out.mutable_data(), v.data(), (size_t)v.rows() * sizeof(int32_t));
    return out;
}

// queryGround: (m, 3) positions -> a structured array with the fields of pwpp_ground_sample
py::array query_ground(PatchWorkpp &self, py::array positions) {
    py::array_t<float, py::array::c_style | py::array::forcecast> a = py::array_t<float, py::array::c_style | py::array::forcecast>::ensure(positions);
    if (!a || a.ndim() != 2 || a.shape(1) != 3) throw py::value_error("queryGround expects an (m, 3) array");
    const int m = (int)a.shape(0);
    std::vector<pwpp_ground_sample> v;
    {
        const float *data = a.data();
        py::gil_scoped_release release;
        v = self.queryGround(data, m);
    }
    py::list fields;
    fields.append(py::make_tuple("patch", "<i4"));
    fields.append(py::make_tuple("decision", "<i4"));
    fields.append(py::make_tuple("ground_z", "<f4"));
    fields.append(py::make_tuple("distance", "<f4"));
    py::array out(py::dtype::from_args(fields), std::vector<py::ssize_t>{(py::ssize_t)m});
    if (m > 0) std::memcpy(out.mutable_data(), v.data(), (size_t)m * sizeof(pwpp_ground_sample));
    return out;
}

// setInputTransform: (3, 4) = [R | t], or (4, 4) homogeneous with the last row 0 0 0 1; None turns the transform off
void set_input_transform(PatchWorkpp &self, py::object T) {
    if (T.is_none()) return self.setInputTransform(nullptr);
    py::array_t<float, py::array::c_style | py::array::forcecast> a = py::array_t<float, py::array::c_style | py::array::forcecast>::ensure(T);
    if (!a || a.ndim() != 2 || a.shape(1) != 4 || (a.shape(0) != 3 && a.shape(0) != 4))
        throw py::value_error("setInputTransform expects a (3, 4) or (4, 4) array");
    const float *v = a.data();
    if (a.shape(0) == 4 && !(v[12] == 0.0f && v[13] == 0.0f && v[14] == 0.0f && v[15] == 1.0f))
        throw py::value_error("setInputTransform: the last row of a (4, 4) transform must be 0 0 0 1");
    self.setInputTransform(v);  // (the first twelve floats of either shape)
}

void estimate_ground(PatchWorkpp &self, py::array cloud) {
    if (cloud.ndim() != 2) throw py::value_error("estimateGround expects a 2-D array (N, 3|4)");
    // F-contiguous float32 is consumed as column-major (the layout Eigen::MatrixXf would have),
    // everything else is brought to C-contiguous float32 (no copy when it already is)
    const bool f_order = (cloud.flags() & py::array::f_style) && !(cloud.flags() & py::array::c_style) &&
                         cloud.dtype().is(py::dtype::of<float>());
    py::array a;
    if (f_order)
        a = py::array_t<float, py::array::f_style>::ensure(cloud);
    else
        a = py::array_t<float, py::array::c_style | py::array::forcecast>::ensure(cloud);
    if (!a) throw py::value_error("estimateGround: cannot convert the input to float32");
    const float *data = static_cast<const float *>(a.data());
    const int rows = (int)a.shape(0), cols = (int)a.shape(1);
    py::gil_scoped_release release;
    self.estimateGround(data, rows, cols, !f_order);
}

}  // namespace

#define PWPP_FIELD(name) cls.def_readwrite(#name, &Params::name)

// (step, slope, rough, count, cost) of a terrain call as (ny, nx) arrays
template <class T>
py::array_t<T> terrain_image(const std::vector<T> &v, int nx, int ny) {
    py::array_t<T> a({(py::ssize_t)ny, (py::ssize_t)nx});
    if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(T));
    return a;
}
template <class Terrain>
py::tuple terrain_tuple(const Terrain &t) {
    return py::make_tuple(terrain_image(t.step, t.nx, t.ny), terrain_image(t.slope, t.nx, t.ny), terrain_image(t.rough, t.nx, t.ny),
                          terrain_image(t.count, t.nx, t.ny), terrain_image(t.cost, t.nx, t.ny));
}

// (reach, from) of a reach call as (ny, nx) arrays
template <class Reach>
py::tuple reach_tuple(const Reach &r) {
    return py::make_tuple(terrain_image(r.reach, r.nx, r.ny), terrain_image(r.from, r.nx, r.ny));
}

// (rows (n, 8) int32 -- status, cells, cost, edge_steps, corner_steps, max_term, min_dist2, waypoints --, cells (n, max_cells), waypoints
// (n, max_waypoints), waypoints_xy (n, max_waypoints, 2)) of a routes call
template <class Routes>
py::tuple routes_tuple(const Routes &r) {
    py::array_t<int32_t> rows({(py::ssize_t)r.n, (py::ssize_t)8}), cells({(py::ssize_t)r.n, (py::ssize_t)r.max_cells}), wps({(py::ssize_t)r.n, (py::ssize_t)r.max_waypoints});
    py::array_t<double> xy({(py::ssize_t)r.n, (py::ssize_t)r.max_waypoints, (py::ssize_t)2});
    if (!r.rows.empty()) std::memcpy(rows.mutable_data(), r.rows.data(), r.rows.size() * sizeof(r.rows[0]));
    std::copy(r.cells.begin(), r.cells.end(), cells.mutable_data());
    std::copy(r.waypoints.begin(), r.waypoints.end(), wps.mutable_data());
    std::copy(r.waypoints_xy.begin(), r.waypoints_xy.end(), xy.mutable_data());
    return py::make_tuple(rows, cells, wps, xy);
}
// n x {x, y} positions in metres from any sequence of numbers
std::vector<double> positions_of(const py::object &xy) {
    const auto a = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(xy);
    if (!a || a.size() % 2 != 0) throw std::invalid_argument("starts_xy: n x {x, y} expected");
    return std::vector<double>(a.data(), a.data() + a.size());
}

// (pose rows (n_traj, n_steps, 8) int32 -- status, covered, outside, blocked, unknown, max_term, min_dist2, hit --, trajectory rows (n_traj, 8)
// int32 -- first_hit, free_steps, last, max_term, sum_term, unknown, min_dist2, reach_last) of a footprint call
template <class Footprints>
py::tuple footprints_tuple(const Footprints &r) {
    py::array_t<int32_t> poses({(py::ssize_t)r.n_traj, (py::ssize_t)r.n_steps, (py::ssize_t)8}), trajs({(py::ssize_t)r.n_traj, (py::ssize_t)8});
    if (!r.poses.empty()) std::memcpy(poses.mutable_data(), r.poses.data(), r.poses.size() * sizeof(r.poses[0]));
    if (!r.trajectories.empty()) std::memcpy(trajs.mutable_data(), r.trajectories.data(), r.trajectories.size() * sizeof(r.trajectories[0]));
    return py::make_tuple(poses, trajs);
}

// (cost, why) of a costmap call as (ny, nx) arrays
template <class Costmap>
py::tuple costmap_tuple(const Costmap &c) {
    return py::make_tuple(terrain_image(c.cost, c.nx, c.ny), terrain_image(c.why, c.nx, c.ny));
}

// the inflation table of a costmap call from any sequence of integers 0 .. 255
std::vector<uint8_t> curve_of(const py::object &curve) {
    if (curve.is_none()) return {};
    const auto a = py::array_t<uint8_t, py::array::c_style | py::array::forcecast>::ensure(curve);
    if (!a) throw std::invalid_argument("curve: a sequence of bytes expected");
    return std::vector<uint8_t>(a.data(), a.data() + a.size());
}

PYBIND11_MODULE(pypatchworkpp, m) {
    m.doc() = "Python Patchwork++ (MI355X / HIP backend)";
    m.attr("__version__") = "0.0.1";
    m.attr("backend") = "hip-gfx950";

    {
        py::class_<Params> cls(m, "Parameters");
        cls.def(py::init<>());
        PWPP_FIELD(verbose);
        PWPP_FIELD(enable_RNR);
        PWPP_FIELD(enable_RVPF);
        PWPP_FIELD(enable_TGR);
        PWPP_FIELD(num_iter);
        PWPP_FIELD(num_lpr);
        PWPP_FIELD(num_min_pts);
        PWPP_FIELD(num_zones);
        PWPP_FIELD(num_rings_of_interest);
        PWPP_FIELD(RNR_ver_angle_thr);
        PWPP_FIELD(RNR_intensity_thr);
        PWPP_FIELD(sensor_height);
        PWPP_FIELD(th_seeds);
        PWPP_FIELD(th_dist);
        PWPP_FIELD(th_seeds_v);
        PWPP_FIELD(th_dist_v);
        PWPP_FIELD(max_range);
        PWPP_FIELD(min_range);
        PWPP_FIELD(uprightness_thr);
        PWPP_FIELD(adaptive_seed_selection_margin);
        PWPP_FIELD(intensity_thr);
        PWPP_FIELD(num_sectors_each_zone);
        PWPP_FIELD(num_rings_each_zone);
        PWPP_FIELD(max_flatness_storage);
        PWPP_FIELD(max_elevation_storage);
        PWPP_FIELD(elevation_thr);
        PWPP_FIELD(flatness_thr);
    }

    PYBIND11_NUMPY_DTYPE(pwpp_obstacle_cluster, first_cell, cells, points, ix_min, ix_max, iy_min, iy_max, top, sum_ix, sum_iy);

    PYBIND11_NUMPY_DTYPE(pwpp_cluster_link, other, overlap, cells, links);
    PYBIND11_NUMPY_DTYPE(pwpp_cluster_evidence, sum, cells, landed, occupied, free, unknown, verdict);
    PYBIND11_NUMPY_DTYPE(pwpp_obstacle_box, points, pad_, mean_x, mean_y, cx, cy, ax, ay, length, width, sigma_long, sigma_short, h_min, h_max, z_min,
                         z_max);
    PYBIND11_NUMPY_DTYPE(pwpp_obstacle_hull, points, n_vertices, stored, rect_edge, area2, qx_min, qx_max, qy_min, qy_max, cx, cy, ax, ay, length, width);

    py::class_<PatchWorkpp::FusedObstacleMap>(m, "FusedObstacleMap")  // the caller's persistent map of updateObstacleMap
        .def(py::init<>())
        .def_readwrite("x0", &PatchWorkpp::FusedObstacleMap::x0)
        .def_readwrite("y0", &PatchWorkpp::FusedObstacleMap::y0)
        .def_readwrite("cell", &PatchWorkpp::FusedObstacleMap::cell)
        .def_readwrite("nx", &PatchWorkpp::FusedObstacleMap::nx)
        .def_readwrite("ny", &PatchWorkpp::FusedObstacleMap::ny)
        .def_readwrite("hit", &PatchWorkpp::FusedObstacleMap::hit)
        .def_readwrite("miss", &PatchWorkpp::FusedObstacleMap::miss)
        .def_readwrite("l_min", &PatchWorkpp::FusedObstacleMap::l_min)
        .def_readwrite("l_max", &PatchWorkpp::FusedObstacleMap::l_max)
        .def_readwrite("occupied_at", &PatchWorkpp::FusedObstacleMap::occupied_at)
        .def_readwrite("free_at", &PatchWorkpp::FusedObstacleMap::free_at);

    py::class_<PatchWorkpp::FusedElevationMap>(m, "FusedElevationMap")  // the caller's persistent map of updateElevationMap
        .def(py::init<>())
        .def_readwrite("x0", &PatchWorkpp::FusedElevationMap::x0)
        .def_readwrite("y0", &PatchWorkpp::FusedElevationMap::y0)
        .def_readwrite("cell", &PatchWorkpp::FusedElevationMap::cell)
        .def_readwrite("nx", &PatchWorkpp::FusedElevationMap::nx)
        .def_readwrite("ny", &PatchWorkpp::FusedElevationMap::ny)
        .def_readwrite("n_max", &PatchWorkpp::FusedElevationMap::n_max);

    py::class_<PatchWorkpp::TerrainParams>(m, "TerrainParams")  // the window and the limits of getTerrain and fusedTerrain
        .def(py::init<>())
        .def_readwrite("radius", &PatchWorkpp::TerrainParams::radius)
        .def_readwrite("min_known", &PatchWorkpp::TerrainParams::min_known)
        .def_readwrite("step_max", &PatchWorkpp::TerrainParams::step_max)
        .def_readwrite("slope_max", &PatchWorkpp::TerrainParams::slope_max)
        .def_readwrite("rough_max", &PatchWorkpp::TerrainParams::rough_max);

    py::class_<PatchWorkpp::RouteParams>(m, "RouteParams")  // the list limits and the shortcut rule of getRoutes and planRoutes
        .def(py::init<>())
        .def_readwrite("max_cells", &PatchWorkpp::RouteParams::max_cells)
        .def_readwrite("max_waypoints", &PatchWorkpp::RouteParams::max_waypoints)
        .def_readwrite("look", &PatchWorkpp::RouteParams::look)
        .def_readwrite("line_cost", &PatchWorkpp::RouteParams::line_cost);
    py::class_<PatchWorkpp::FootprintParams>(m, "FootprintParams")  // the vehicle's rectangle in metres, its padding in ticks, the flag of checkFootprints
        .def(py::init<>())
        .def_readwrite("front", &PatchWorkpp::FootprintParams::front)
        .def_readwrite("rear", &PatchWorkpp::FootprintParams::rear)
        .def_readwrite("half_width", &PatchWorkpp::FootprintParams::half_width)
        .def_readwrite("pad", &PatchWorkpp::FootprintParams::pad)
        .def_readwrite("outside_blocks", &PatchWorkpp::FootprintParams::outside_blocks);
    py::class_<PatchWorkpp::ReachParams>(m, "ReachParams")  // the step costs and the limits of getReach and fusedReach
        .def(py::init<>())
        .def_readwrite("base", &PatchWorkpp::ReachParams::base)
        .def_readwrite("lethal", &PatchWorkpp::ReachParams::lethal)
        .def_readwrite("unknown", &PatchWorkpp::ReachParams::unknown)
        .def_readwrite("clearance2", &PatchWorkpp::ReachParams::clearance2)
        .def_readwrite("max_reach", &PatchWorkpp::ReachParams::max_reach);

    py::class_<PatchWorkpp::CostmapParams>(m, "CostmapParams")  // the layers and the unknown rules of getCostmap and fusedCostmap
        .def(py::init<>())
        .def_readwrite("layers", &PatchWorkpp::CostmapParams::layers)
        .def_readwrite("occupancy_unknown", &PatchWorkpp::CostmapParams::occupancy_unknown)
        .def_readwrite("terrain_unknown", &PatchWorkpp::CostmapParams::terrain_unknown)
        .def_readwrite("unknown_below", &PatchWorkpp::CostmapParams::unknown_below);

    py::class_<PatchWorkpp>(m, "patchworkpp")
        .def(py::init<Params>())
        .def(py::init<Params, int>(), py::arg("params"), py::arg("device"))
        .def("estimateGround", &estimate_ground)
        .def("getHeight", &PatchWorkpp::getHeight)
        .def("getTimeTaken", &PatchWorkpp::getTimeTaken)
        .def("setReferenceOrder", &PatchWorkpp::setReferenceOrder, py::arg("on"))
        .def("setCloudOrder", &PatchWorkpp::setCloudOrder, py::arg("on"))
        .def("setLabels", &PatchWorkpp::setLabels, py::arg("on"))
        .def("getLabels", [](PatchWorkpp &s) { return to_numpy(s.labelList()); })
        .def("setPointPlanes", &PatchWorkpp::setPointPlanes, py::arg("on"))
        .def("getPointPatches", [](PatchWorkpp &s) { return to_numpy(s.pointPatchList()); })
        .def("getPointDistances", [](PatchWorkpp &s) { return to_numpy(s.pointDistanceList()); })
        .def("setPointRecords", &PatchWorkpp::setPointRecords, py::arg("on"))
        .def("setInputTransform", &set_input_transform, py::arg("T").none(true))
        .def("queryGround", &query_ground, py::arg("positions"))
        .def("getElevationMap",
             [](PatchWorkpp &s, double x0, double y0, double cell, int nx, int ny, bool ground_only) {
                 return to_numpy(s.elevationMapRows(x0, y0, cell, nx, ny, ground_only));
             },
             py::arg("x0"), py::arg("y0"), py::arg("cell"), py::arg("nx"), py::arg("ny"), py::arg("ground_only") = false)
        .def("getObstacleMap",
             [](PatchWorkpp &s, double x0, double y0, double cell, int nx, int ny, float h_min, float h_max, bool ground_only) {
                 const PatchWorkpp::ObstacleMap m = s.obstacleMapRows(x0, y0, cell, nx, ny, h_min, h_max, ground_only);
                 py::array_t<int32_t> count({(py::ssize_t)m.top.rows(), (py::ssize_t)m.top.cols()});
                 if (!m.count.empty()) std::memcpy(count.mutable_data(), m.count.data(), m.count.size() * sizeof(int32_t));
                 return py::make_tuple(count, to_numpy(m.top));
             },
             py::arg("x0"), py::arg("y0"), py::arg("cell"), py::arg("nx"), py::arg("ny"), py::arg("h_min"), py::arg("h_max"),
             py::arg("ground_only") = false)
        .def("getObstacleClusters",
             [](PatchWorkpp &s, double x0, double y0, double cell, int nx, int ny, float h_min, float h_max, int min_count, int connectivity,
                bool ground_only) {
                 const PatchWorkpp::ObstacleClusters c = s.getObstacleClusters(x0, y0, cell, nx, ny, h_min, h_max, min_count, connectivity, ground_only);
                 py::array_t<int32_t> label({(py::ssize_t)(ny > 0 ? ny : 0), (py::ssize_t)(nx > 0 ? nx : 0)});
                 if (!c.label.empty()) std::memcpy(label.mutable_data(), c.label.data(), c.label.size() * sizeof(int32_t));
                 py::array_t<pwpp_obstacle_cluster> table((py::ssize_t)c.clusters.size());  // a structured array: one field per member
                 if (!c.clusters.empty()) std::memcpy(table.mutable_data(), c.clusters.data(), c.clusters.size() * sizeof(pwpp_obstacle_cluster));
                 return py::make_tuple(label, table, c.count);
             },
             py::arg("x0"), py::arg("y0"), py::arg("cell"), py::arg("nx"), py::arg("ny"), py::arg("h_min"), py::arg("h_max"),
             py::arg("min_count") = 1, py::arg("connectivity") = 8, py::arg("ground_only") = false)
        .def("getObstacleDistances",
             [](PatchWorkpp &s, double x0, double y0, double cell, int nx, int ny, float h_min, float h_max, int min_count, int max_dist, bool ground_only) {
                 const PatchWorkpp::ObstacleDistances d = s.getObstacleDistances(x0, y0, cell, nx, ny, h_min, h_max, min_count, max_dist, ground_only);
                 py::array_t<int32_t> dist2({(py::ssize_t)d.metres.rows(), (py::ssize_t)d.metres.cols()});
                 py::array_t<int32_t> nearest({(py::ssize_t)d.metres.rows(), (py::ssize_t)d.metres.cols()});
                 if (!d.dist2.empty()) std::memcpy(dist2.mutable_data(), d.dist2.data(), d.dist2.size() * sizeof(int32_t));
                 if (!d.nearest.empty()) std::memcpy(nearest.mutable_data(), d.nearest.data(), d.nearest.size() * sizeof(int32_t));
                 return py::make_tuple(dist2, nearest, to_numpy(d.metres));
             },
             py::arg("x0"), py::arg("y0"), py::arg("cell"), py::arg("nx"), py::arg("ny"), py::arg("h_min"), py::arg("h_max"),
             py::arg("min_count") = 1, py::arg("max_dist") = 0, py::arg("ground_only") = false)
        .def("getObstacleVisibility",
             [](PatchWorkpp &s, double x0, double y0, double cell, int nx, int ny, float h_min, float h_max, int min_count, int max_range, double origin_x,
                double origin_y, bool ground_only) {
                 const PatchWorkpp::ObstacleVisibility v =
                     s.getObstacleVisibility(x0, y0, cell, nx, ny, h_min, h_max, min_count, max_range, origin_x, origin_y, ground_only);
                 py::array_t<int32_t> first({(py::ssize_t)v.ny, (py::ssize_t)v.nx});
                 py::array_t<int8_t> occupancy({(py::ssize_t)v.ny, (py::ssize_t)v.nx});
                 if (!v.first.empty()) std::memcpy(first.mutable_data(), v.first.data(), v.first.size() * sizeof(int32_t));
                 if (!v.occupancy.empty()) std::memcpy(occupancy.mutable_data(), v.occupancy.data(), v.occupancy.size());
                 return py::make_tuple(first, occupancy);
             },
             py::arg("x0"), py::arg("y0"), py::arg("cell"), py::arg("nx"), py::arg("ny"), py::arg("h_min"), py::arg("h_max"),
             py::arg("min_count") = 1, py::arg("max_range") = 0, py::arg("origin_x") = 0.0, py::arg("origin_y") = 0.0, py::arg("ground_only") = false)
        .def("getObstacleViewshed",
             [](PatchWorkpp &s, double x0, double y0, double cell, int nx, int ny, float h_min, float h_max, int min_count, int min_seen, int max_range,
                double origin_x, double origin_y, double origin_z, bool ground_only) {
                 const PatchWorkpp::ObstacleViewshed v =
                     s.getObstacleViewshed(x0, y0, cell, nx, ny, h_min, h_max, min_count, min_seen, max_range, origin_x, origin_y, origin_z, ground_only);
                 py::array_t<int32_t> first({(py::ssize_t)v.ny, (py::ssize_t)v.nx});
                 py::array_t<int32_t> shadow({(py::ssize_t)v.ny, (py::ssize_t)v.nx});
                 py::array_t<int8_t> occupancy({(py::ssize_t)v.ny, (py::ssize_t)v.nx});
                 if (!v.first.empty()) std::memcpy(first.mutable_data(), v.first.data(), v.first.size() * sizeof(int32_t));
                 if (!v.shadow.empty()) std::memcpy(shadow.mutable_data(), v.shadow.data(), v.shadow.size() * sizeof(int32_t));
                 if (!v.occupancy.empty()) std::memcpy(occupancy.mutable_data(), v.occupancy.data(), v.occupancy.size());
                 return py::make_tuple(first, shadow, occupancy);
             },
             py::arg("x0"), py::arg("y0"), py::arg("cell"), py::arg("nx"), py::arg("ny"), py::arg("h_min"), py::arg("h_max"),
             py::arg("min_count") = 1, py::arg("min_seen") = 1, py::arg("max_range") = 0, py::arg("origin_x") = 0.0, py::arg("origin_y") = 0.0,
             py::arg("origin_z") = 0.0, py::arg("ground_only") = false)
        .def("getBeamClearance",
             [](PatchWorkpp &s, double x0, double y0, double cell, int nx, int ny, int min_pass, double clearance, int max_range, double origin_x,
                double origin_y, double origin_z, int which, bool ground_only, py::object occupancy_in) {
                 std::vector<int8_t> base;
                 if (!occupancy_in.is_none()) {
                     const auto a = py::array_t<int8_t, py::array::c_style | py::array::forcecast>::ensure(occupancy_in);
                     if (!a) throw std::invalid_argument("getBeamClearance: occupancy_in must be an int8 array");
                     base.assign(a.data(), a.data() + a.size());
                 }
                 const PatchWorkpp::BeamClearance v =
                     s.getBeamClearance(x0, y0, cell, nx, ny, min_pass, clearance, max_range, origin_x, origin_y, origin_z, which, ground_only, base);
                 py::array_t<uint32_t> passes({(py::ssize_t)v.ny, (py::ssize_t)v.nx});
                 py::array_t<int32_t> low({(py::ssize_t)v.ny, (py::ssize_t)v.nx});
                 py::array_t<int8_t> occupancy({(py::ssize_t)v.ny, (py::ssize_t)v.nx});
                 if (!v.passes.empty()) std::memcpy(passes.mutable_data(), v.passes.data(), v.passes.size() * sizeof(uint32_t));
                 if (!v.low.empty()) std::memcpy(low.mutable_data(), v.low.data(), v.low.size() * sizeof(int32_t));
                 if (!v.occupancy.empty()) std::memcpy(occupancy.mutable_data(), v.occupancy.data(), v.occupancy.size());
                 return py::make_tuple(passes, low, occupancy);
             },
             py::arg("x0"), py::arg("y0"), py::arg("cell"), py::arg("nx"), py::arg("ny"), py::arg("min_pass") = 1, py::arg("clearance") = 0.3,
             py::arg("max_range") = 0, py::arg("origin_x") = 0.0, py::arg("origin_y") = 0.0, py::arg("origin_z") = 0.0, py::arg("which") = 1,
             py::arg("ground_only") = false, py::arg("occupancy_in") = py::none())
        .def("updateObstacleMap",
             [](PatchWorkpp &s, PatchWorkpp::FusedObstacleMap &map, const std::array<double, 6> &pose, double x0, double y0, double cell, int nx, int ny,
                float h_min, float h_max, int min_count, int max_range, double origin_x, double origin_y, int shift_x, int shift_y) {
                 s.updateObstacleMap(map, pose.data(), x0, y0, cell, nx, ny, h_min, h_max, min_count, max_range, origin_x, origin_y, shift_x, shift_y);
                 py::array_t<int16_t> log_odds({(py::ssize_t)map.ny, (py::ssize_t)map.nx});
                 py::array_t<int8_t> occupancy({(py::ssize_t)map.ny, (py::ssize_t)map.nx});
                 if (!map.log_odds.empty()) std::memcpy(log_odds.mutable_data(), map.log_odds.data(), map.log_odds.size() * sizeof(int16_t));
                 if (!map.occupancy.empty()) std::memcpy(occupancy.mutable_data(), map.occupancy.data(), map.occupancy.size());
                 return py::make_tuple(log_odds, occupancy);
             },
             py::arg("map"), py::arg("pose"), py::arg("x0"), py::arg("y0"), py::arg("cell"), py::arg("nx"), py::arg("ny"), py::arg("h_min"),
             py::arg("h_max"), py::arg("min_count") = 1, py::arg("max_range") = 0, py::arg("origin_x") = 0.0, py::arg("origin_y") = 0.0,
             py::arg("shift_x") = 0, py::arg("shift_y") = 0)
        .def("updateElevationMap",
             [](PatchWorkpp &s, PatchWorkpp::FusedElevationMap &map, const std::array<double, 6> &pose, double z_offset, double x0, double y0, double cell,
                int nx, int ny, bool ground_only, int shift_x, int shift_y) {
                 s.updateElevationMap(map, pose.data(), z_offset, x0, y0, cell, nx, ny, ground_only, shift_x, shift_y);
                 py::array_t<int32_t> sum({(py::ssize_t)map.ny, (py::ssize_t)map.nx});
                 py::array_t<int16_t> n({(py::ssize_t)map.ny, (py::ssize_t)map.nx});
                 if (!map.sum.empty()) std::memcpy(sum.mutable_data(), map.sum.data(), map.sum.size() * sizeof(int32_t));
                 if (!map.n.empty()) std::memcpy(n.mutable_data(), map.n.data(), map.n.size() * sizeof(int16_t));
                 return py::make_tuple(sum, n, to_numpy(PatchWorkpp::fusedElevationRows(map)));
             },
             py::arg("map"), py::arg("pose"), py::arg("z_offset"), py::arg("x0"), py::arg("y0"), py::arg("cell"), py::arg("nx"), py::arg("ny"),
             py::arg("ground_only") = false, py::arg("shift_x") = 0, py::arg("shift_y") = 0)
        .def("getFusedElevation", [](PatchWorkpp &, const PatchWorkpp::FusedElevationMap &map) { return to_numpy(PatchWorkpp::fusedElevationRows(map)); },
             py::arg("map"))
        .def("getTerrain",
             [](PatchWorkpp &s, double x0, double y0, double cell, int nx, int ny, const PatchWorkpp::TerrainParams &params, bool ground_only) {
                 return terrain_tuple(s.getTerrain(x0, y0, cell, nx, ny, params, ground_only));
             },
             py::arg("x0"), py::arg("y0"), py::arg("cell"), py::arg("nx"), py::arg("ny"), py::arg("params") = PatchWorkpp::TerrainParams(),
             py::arg("ground_only") = false)
        .def("fusedTerrain",
             [](PatchWorkpp &s, const PatchWorkpp::FusedElevationMap &map, const PatchWorkpp::TerrainParams &params) {
                 return terrain_tuple(s.fusedTerrain(map, params));
             },
             py::arg("map"), py::arg("params") = PatchWorkpp::TerrainParams())
        .def("getReach",
             [](PatchWorkpp &s, double x0, double y0, double cell, int nx, int ny, const PatchWorkpp::TerrainParams &terrain_params,
                const PatchWorkpp::ReachParams &reach_params, double source_x, double source_y, bool ground_only) {
                 return reach_tuple(s.getReach(x0, y0, cell, nx, ny, terrain_params, reach_params, source_x, source_y, ground_only));
             },
             py::arg("x0"), py::arg("y0"), py::arg("cell"), py::arg("nx"), py::arg("ny"), py::arg("terrain_params") = PatchWorkpp::TerrainParams(),
             py::arg("reach_params") = PatchWorkpp::ReachParams(), py::arg("source_x") = 0.0, py::arg("source_y") = 0.0, py::arg("ground_only") = false)
        .def("fusedReach",
             [](PatchWorkpp &s, const PatchWorkpp::FusedElevationMap &map, const PatchWorkpp::TerrainParams &terrain_params,
                const PatchWorkpp::ReachParams &reach_params, double source_x, double source_y) {
                 return reach_tuple(s.fusedReach(map, terrain_params, reach_params, source_x, source_y));
             },
             py::arg("map"), py::arg("terrain_params") = PatchWorkpp::TerrainParams(), py::arg("reach_params") = PatchWorkpp::ReachParams(),
             py::arg("source_x") = 0.0, py::arg("source_y") = 0.0)
        .def("getRoutes",
             [](PatchWorkpp &s, double x0, double y0, double cell, int nx, int ny, const py::object &starts_xy, const PatchWorkpp::TerrainParams &terrain_params,
                const PatchWorkpp::ReachParams &reach_params, const PatchWorkpp::RouteParams &route_params, double source_x, double source_y, bool ground_only) {
                 return routes_tuple(s.getRoutes(x0, y0, cell, nx, ny, positions_of(starts_xy), terrain_params, reach_params, route_params, source_x, source_y, ground_only));
             },
             py::arg("x0"), py::arg("y0"), py::arg("cell"), py::arg("nx"), py::arg("ny"), py::arg("starts_xy"), py::arg("terrain_params") = PatchWorkpp::TerrainParams(),
             py::arg("reach_params") = PatchWorkpp::ReachParams(), py::arg("route_params") = PatchWorkpp::RouteParams(), py::arg("source_x") = 0.0,
             py::arg("source_y") = 0.0, py::arg("ground_only") = false)
        .def("planRoutes",
             [](PatchWorkpp &s, const py::object &cost, double x0, double y0, double cell, int nx, int ny, const py::object &starts_xy,
                const PatchWorkpp::ReachParams &reach_params, const PatchWorkpp::RouteParams &route_params, double source_x, double source_y) {
                 const auto c = py::array_t<int8_t, py::array::c_style | py::array::forcecast>::ensure(cost);
                 if (!c) throw std::invalid_argument("cost: an int8 image expected");
                 return routes_tuple(s.planRoutes(std::vector<int8_t>(c.data(), c.data() + c.size()), x0, y0, cell, nx, ny, positions_of(starts_xy), reach_params,
                                                  route_params, source_x, source_y));
             },
             py::arg("cost"), py::arg("x0"), py::arg("y0"), py::arg("cell"), py::arg("nx"), py::arg("ny"), py::arg("starts_xy"),
             py::arg("reach_params") = PatchWorkpp::ReachParams(), py::arg("route_params") = PatchWorkpp::RouteParams(), py::arg("source_x") = 0.0,
             py::arg("source_y") = 0.0)
        .def("checkFootprints",
             [](PatchWorkpp &s, const py::object &cost, double x0, double y0, double cell, int nx, int ny, const py::object &poses_xyyaw,
                const PatchWorkpp::FootprintParams &footprint_params, const PatchWorkpp::ReachParams &reach_params, const py::object &reach) {
                 const auto c = py::array_t<int8_t, py::array::c_style | py::array::forcecast>::ensure(cost);
                 if (!c) throw std::invalid_argument("cost: an int8 image expected");
                 const auto q = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(poses_xyyaw);
                 if (!q || q.ndim() != 3 || q.shape(2) != 3) throw std::invalid_argument("poses_xyyaw: (n_traj, n_steps, 3) expected");
                 std::vector<int32_t> field;
                 if (!reach.is_none()) {
                     const auto f = py::array_t<int32_t, py::array::c_style | py::array::forcecast>::ensure(reach);
                     if (!f) throw std::invalid_argument("reach: an int32 image expected");
                     field.assign(f.data(), f.data() + f.size());
                 }
                 return footprints_tuple(s.checkFootprints(std::vector<int8_t>(c.data(), c.data() + c.size()), x0, y0, cell, nx, ny,
                                                           std::vector<double>(q.data(), q.data() + q.size()), (int)q.shape(1), footprint_params, reach_params, field));
             },
             py::arg("cost"), py::arg("x0"), py::arg("y0"), py::arg("cell"), py::arg("nx"), py::arg("ny"), py::arg("poses_xyyaw"),
             py::arg("footprint_params") = PatchWorkpp::FootprintParams(), py::arg("reach_params") = PatchWorkpp::ReachParams(), py::arg("reach") = py::none())
        .def_static("inflationCurve",
                    [](double cell, double inscribed, double radius, double decay, int peak) {
                        const std::vector<uint8_t> c = PatchWorkpp::inflationCurve(cell, inscribed, radius, decay, peak);
                        py::array_t<uint8_t> out((py::ssize_t)c.size());
                        std::copy(c.begin(), c.end(), out.mutable_data());
                        return out;
                    },
                    py::arg("cell"), py::arg("inscribed"), py::arg("radius"), py::arg("decay"), py::arg("peak") = 99)
        .def("getCostmap",
             [](PatchWorkpp &s, double x0, double y0, double cell, int nx, int ny, float h_min, float h_max, const py::object &curve,
                const PatchWorkpp::CostmapParams &params, const PatchWorkpp::TerrainParams &terrain_params, int min_count, int max_range, double origin_x,
                double origin_y, bool ground_only) {
                 return costmap_tuple(s.getCostmap(x0, y0, cell, nx, ny, h_min, h_max, curve_of(curve), params, terrain_params, min_count, max_range, origin_x,
                                                   origin_y, ground_only));
             },
             py::arg("x0"), py::arg("y0"), py::arg("cell"), py::arg("nx"), py::arg("ny"), py::arg("h_min"), py::arg("h_max"), py::arg("curve") = py::none(),
             py::arg("params") = PatchWorkpp::CostmapParams(), py::arg("terrain_params") = PatchWorkpp::TerrainParams(), py::arg("min_count") = 1,
             py::arg("max_range") = 0, py::arg("origin_x") = 0.0, py::arg("origin_y") = 0.0, py::arg("ground_only") = false)
        .def("fusedCostmap",
             [](PatchWorkpp &s, const PatchWorkpp::FusedObstacleMap &map, const PatchWorkpp::FusedElevationMap *elevation, const py::object &curve,
                const PatchWorkpp::CostmapParams &params, const PatchWorkpp::TerrainParams &terrain_params) {
                 return costmap_tuple(s.fusedCostmap(map, elevation, curve_of(curve), params, terrain_params));
             },
             py::arg("map"), py::arg("elevation") = static_cast<const PatchWorkpp::FusedElevationMap *>(nullptr), py::arg("curve") = py::none(),
             py::arg("params") = PatchWorkpp::CostmapParams(), py::arg("terrain_params") = PatchWorkpp::TerrainParams())
        .def("matchObstacleMap",
             [](PatchWorkpp &s, const PatchWorkpp::FusedObstacleMap &map, const std::vector<std::array<double, 6>> &candidates, int wx, int wy, double x0,
                double y0, double cell, int nx, int ny, float h_min, float h_max, int min_count, int max_range, double origin_x, double origin_y) {
                 const PatchWorkpp::ObstacleMatch r =
                     s.matchObstacleMap(map, candidates.empty() ? nullptr : candidates.front().data(), (int)candidates.size(), wx, wy, x0, y0, cell, nx, ny,
                                        h_min, h_max, min_count, max_range, origin_x, origin_y);
                 return py::make_tuple(r.candidate, r.sx, r.sy, r.score, r.cells, std::array<double, 6>{r.pose[0], r.pose[1], r.pose[2], r.pose[3], r.pose[4], r.pose[5]});
             },
             py::arg("map"), py::arg("candidates"), py::arg("wx"), py::arg("wy"), py::arg("x0"), py::arg("y0"), py::arg("cell"), py::arg("nx"),
             py::arg("ny"), py::arg("h_min"), py::arg("h_max"), py::arg("min_count") = 1, py::arg("max_range") = 0, py::arg("origin_x") = 0.0,
             py::arg("origin_y") = 0.0)
        .def("getObstacleBoxes",
             [](PatchWorkpp &s, double x0, double y0, double cell, int nx, int ny, float h_min, float h_max, int min_count, int connectivity,
                bool ground_only) {
                 const PatchWorkpp::ObstacleBoxes b = s.getObstacleBoxes(x0, y0, cell, nx, ny, h_min, h_max, min_count, connectivity, ground_only);
                 py::array_t<int32_t> label({(py::ssize_t)(ny > 0 ? ny : 0), (py::ssize_t)(nx > 0 ? nx : 0)});
                 if (!b.label.empty()) std::memcpy(label.mutable_data(), b.label.data(), b.label.size() * sizeof(int32_t));
                 py::array_t<pwpp_obstacle_cluster> table((py::ssize_t)b.clusters.size());
                 if (!b.clusters.empty()) std::memcpy(table.mutable_data(), b.clusters.data(), b.clusters.size() * sizeof(pwpp_obstacle_cluster));
                 py::array_t<pwpp_obstacle_box> boxes((py::ssize_t)b.boxes.size());
                 if (!b.boxes.empty()) std::memcpy(boxes.mutable_data(), b.boxes.data(), b.boxes.size() * sizeof(pwpp_obstacle_box));
                 return py::make_tuple(label, table, boxes, b.count);
             },
             py::arg("x0"), py::arg("y0"), py::arg("cell"), py::arg("nx"), py::arg("ny"), py::arg("h_min"), py::arg("h_max"),
             py::arg("min_count") = 1, py::arg("connectivity") = 8, py::arg("ground_only") = false)
        .def("getObstacleHulls",
             [](PatchWorkpp &s, double x0, double y0, double cell, int nx, int ny, float h_min, float h_max, int max_vertices, int min_count, int connectivity,
                bool ground_only) {
                 const PatchWorkpp::ObstacleHulls o = s.getObstacleHulls(x0, y0, cell, nx, ny, h_min, h_max, max_vertices, min_count, connectivity, ground_only);
                 py::array_t<int32_t> label({(py::ssize_t)(ny > 0 ? ny : 0), (py::ssize_t)(nx > 0 ? nx : 0)});
                 if (!o.label.empty()) std::memcpy(label.mutable_data(), o.label.data(), o.label.size() * sizeof(int32_t));
                 py::array_t<pwpp_obstacle_cluster> table((py::ssize_t)o.clusters.size());
                 if (!o.clusters.empty()) std::memcpy(table.mutable_data(), o.clusters.data(), o.clusters.size() * sizeof(pwpp_obstacle_cluster));
                 py::array_t<pwpp_obstacle_hull> hulls((py::ssize_t)o.hulls.size());
                 if (!o.hulls.empty()) std::memcpy(hulls.mutable_data(), o.hulls.data(), o.hulls.size() * sizeof(pwpp_obstacle_hull));
                 py::array_t<int32_t> vertices({(py::ssize_t)o.hulls.size(), (py::ssize_t)(max_vertices > 0 ? max_vertices : 0), (py::ssize_t)2});
                 if (!o.vertices.empty()) std::memcpy(vertices.mutable_data(), o.vertices.data(), o.vertices.size() * sizeof(int32_t));
                 return py::make_tuple(label, table, hulls, vertices, o.count);
             },
             py::arg("x0"), py::arg("y0"), py::arg("cell"), py::arg("nx"), py::arg("ny"), py::arg("h_min"), py::arg("h_max"), py::arg("max_vertices") = 32,
             py::arg("min_count") = 1, py::arg("connectivity") = 8, py::arg("ground_only") = false)
        .def("trackObstacleClusters",
             [](PatchWorkpp &s, double x0, double y0, double cell, int nx, int ny, float h_min, float h_max, const std::array<double, 6> &pose, int min_count,
                int connectivity, int max_clusters, int gate, int min_overlap) {
                 const PatchWorkpp::ObstacleTracks t =
                     s.trackObstacleClusters(x0, y0, cell, nx, ny, h_min, h_max, pose.data(), min_count, connectivity, max_clusters, gate, min_overlap);
                 py::array_t<int32_t> label({(py::ssize_t)t.ny, (py::ssize_t)t.nx});
                 if (!t.label.empty()) std::memcpy(label.mutable_data(), t.label.data(), t.label.size() * sizeof(int32_t));
                 py::array_t<pwpp_obstacle_cluster> table((py::ssize_t)t.clusters.size());
                 if (!t.clusters.empty()) std::memcpy(table.mutable_data(), t.clusters.data(), t.clusters.size() * sizeof(pwpp_obstacle_cluster));
                 py::array_t<pwpp_cluster_link> curr_links((py::ssize_t)t.curr_links.size()), prev_links((py::ssize_t)t.prev_links.size());
                 if (!t.curr_links.empty()) std::memcpy(curr_links.mutable_data(), t.curr_links.data(), t.curr_links.size() * sizeof(pwpp_cluster_link));
                 if (!t.prev_links.empty()) std::memcpy(prev_links.mutable_data(), t.prev_links.data(), t.prev_links.size() * sizeof(pwpp_cluster_link));
                 py::array_t<int32_t> ids((py::ssize_t)t.ids.size());
                 if (!t.ids.empty()) std::memcpy(ids.mutable_data(), t.ids.data(), t.ids.size() * sizeof(int32_t));
                 return py::make_tuple(label, table, curr_links, prev_links, ids, t.count, t.pairs);
             },
             py::arg("x0"), py::arg("y0"), py::arg("cell"), py::arg("nx"), py::arg("ny"), py::arg("h_min"), py::arg("h_max"),
             py::arg("pose") = std::array<double, 6>{{1.0, 0.0, 0.0, 0.0, 1.0, 0.0}}, py::arg("min_count") = 1, py::arg("connectivity") = 8,
             py::arg("max_clusters") = 256, py::arg("gate") = 1, py::arg("min_overlap") = 1)
        .def("resetObstacleTracks", [](PatchWorkpp &s) { s.resetObstacleTracks(); })
        .def("getObstacleEvidence",
             [](PatchWorkpp &s, const PatchWorkpp::FusedObstacleMap &map, double x0, double y0, double cell, int nx, int ny, float h_min, float h_max,
                const std::array<double, 6> &pose, int gate, int min_cells, int moving_share, int static_share, py::object occupancy, int min_count,
                int connectivity, int max_clusters) {
                 PatchWorkpp::EvidenceRule rule;
                 rule.gate = gate, rule.min_cells = min_cells, rule.moving_share = moving_share, rule.static_share = static_share;
                 py::array_t<int8_t, py::array::c_style | py::array::forcecast> occ;
                 if (!occupancy.is_none()) {
                     occ = py::array_t<int8_t, py::array::c_style | py::array::forcecast>::ensure(occupancy);
                     if (!occ || occ.size() != (py::ssize_t)(nx > 0 ? nx : 0) * (py::ssize_t)(ny > 0 ? ny : 0) || occ.size() == 0)
                         throw std::invalid_argument("getObstacleEvidence: occupancy must hold ny x nx int8 values");
                 }
                 const PatchWorkpp::ObstacleEvidence e = s.getObstacleEvidence(map, x0, y0, cell, nx, ny, h_min, h_max, pose.data(), rule,
                                                                               occupancy.is_none() ? nullptr : occ.data(), min_count, connectivity, max_clusters);
                 py::array_t<int32_t> label({(py::ssize_t)e.ny, (py::ssize_t)e.nx});
                 if (!e.label.empty()) std::memcpy(label.mutable_data(), e.label.data(), e.label.size() * sizeof(int32_t));
                 py::array_t<pwpp_obstacle_cluster> table((py::ssize_t)e.clusters.size());
                 if (!e.clusters.empty()) std::memcpy(table.mutable_data(), e.clusters.data(), e.clusters.size() * sizeof(pwpp_obstacle_cluster));
                 py::array_t<pwpp_cluster_evidence> rows((py::ssize_t)e.rows.size());  // a structured array: one field per member
                 if (!e.rows.empty()) std::memcpy(rows.mutable_data(), e.rows.data(), e.rows.size() * sizeof(pwpp_cluster_evidence));
                 py::array_t<int8_t> cell_class({(py::ssize_t)e.ny, (py::ssize_t)e.nx});
                 if (!e.cell_class.empty()) std::memcpy(cell_class.mutable_data(), e.cell_class.data(), e.cell_class.size());
                 py::object masked = py::none();
                 if (!occupancy.is_none()) {
                     py::array_t<int8_t> bytes({(py::ssize_t)e.ny, (py::ssize_t)e.nx});
                     if (!e.masked.empty()) std::memcpy(bytes.mutable_data(), e.masked.data(), e.masked.size());
                     masked = bytes;
                 }
                 return py::make_tuple(label, table, rows, cell_class, masked, e.count);
             },
             py::arg("map"), py::arg("x0"), py::arg("y0"), py::arg("cell"), py::arg("nx"), py::arg("ny"), py::arg("h_min"), py::arg("h_max"),
             py::arg("pose") = std::array<double, 6>{{1.0, 0.0, 0.0, 0.0, 1.0, 0.0}}, py::arg("gate") = 1, py::arg("min_cells") = 3,
             py::arg("moving_share") = 192, py::arg("static_share") = 192, py::arg("occupancy") = py::none(), py::arg("min_count") = 1,
             py::arg("connectivity") = 8, py::arg("max_clusters") = 256)
        .def("getGroundPoints", [](PatchWorkpp &s) { return to_numpy(s.groundPointRows()); })
        .def("getNongroundPoints", [](PatchWorkpp &s) { return to_numpy(s.nongroundPointRows()); })
        .def("getGround", [](PatchWorkpp &s) { return to_numpy(s.getGround()); })
        .def("getNonground", [](PatchWorkpp &s) { return to_numpy(s.getNonground()); })
        .def("getCenters", [](PatchWorkpp &s) { return to_numpy(s.getCenters()); })
        .def("getNormals", [](PatchWorkpp &s) { return to_numpy(s.getNormals()); })
        .def("getGroundIndices", [](PatchWorkpp &s) { return to_numpy(s.getGroundIndices()); })
        .def("getNongroundIndices", [](PatchWorkpp &s) { return to_numpy(s.getNongroundIndices()); });
}
