/* capi_demo.c -- the C-ABI from plain C99 (what a cgo / JNI / ctypes-style binding sees): one KITTI-layout
 * .bin frame through pwpp_estimate_ground(), counts and the first indices printed; then the frame as a tilted sensor delivers it
 * (pwpp_set_input_transforms), and batches in flight.
 *   gcc -std=c99 -Wall -Werror -I ../../include capi_demo.c -o capi_demo -L ../lib -lpwpp_hip -Wl,-rpath,'$ORIGIN/../lib'
 *   ./capi_demo <frame.bin>
 * Mirrors the read loop of the reference demo (cpp/patchworkpp/examples/demo_visualize.cpp:18-34) and its
 * use of the object (:60-72), through the C entry points that replace each call. */
#include <stdio.h>
#include <stdlib.h>

#include "pwpp.h"

static int fail(const char *what) {
    fprintf(stderr, "%s: %s\n", what, pwpp_last_error());
    return 1;
}

int main(int argc, char **argv) {
    pwpp_params params;
    pwpp_handle *h = NULL;
    FILE *f;
    long bytes;
    int n;
    float *pts;
    int32_t n_ground = 0, n_nonground = 0, n_patches = 0;
    int32_t *ground;

    if (pwpp_params_default(&params) != PWPP_OK) return fail("pwpp_params_default"); /* Params(), patchworkpp.h:79-111 */
    params.verbose = 0;
    if (pwpp_create(&params, 0, &h) != PWPP_OK) {  /* PatchWorkpp(Params), patchworkpp.h:120 */
        /* no GPU: the library says so and does NOT fall back to a CPU path */
        fprintf(stderr, "pwpp_create: %s\n", pwpp_last_error());
        return 2;
    }
    if (argc < 2) {
        fprintf(stderr, "usage: %s <frame.bin>\n", argv[0]);
        pwpp_destroy(h);
        return 1;
    }
    f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 1;
    }
    fseek(f, 0, SEEK_END);
    bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    n = (int)(bytes / (4 * (long)sizeof(float)));  /* x, y, z, intensity */
    pts = (float *)malloc((size_t)n * 4 * sizeof(float));
    if (!pts || fread(pts, 4 * sizeof(float), (size_t)n, f) != (size_t)n) {
        fprintf(stderr, "short read\n");
        return 1;
    }
    fclose(f);

    if (pwpp_estimate_ground(h, pts, n, 4, PWPP_LAYOUT_ROW_MAJOR) != PWPP_OK) return fail("pwpp_estimate_ground"); /* estimateGround(), patchworkpp.cpp:151 */
    if (pwpp_get_counts(h, 0, &n_ground, &n_nonground, &n_patches) != PWPP_OK) return fail("pwpp_get_counts");
    ground = (int32_t *)malloc((size_t)(n_ground > 0 ? n_ground : 1) * sizeof(int32_t));
    if (pwpp_get_ground_indices(h, 0, ground) != PWPP_OK) return fail("pwpp_get_ground_indices");   /* getGroundIndices(), patchworkpp.h:159 */
    printf("points %d ground %d nonground %d patches %d height %.6f time_us %.1f\n", n, (int)n_ground, (int)n_nonground,
           (int)n_patches, pwpp_get_height(h), pwpp_get_time_us(h));
    free(ground);

    /* A route (pwpp_plan_grid, no reference counterpart): 9 x 9 cells of free ground with a wall across column 4 that is open in its
     * last row; the field from the goal at (8, 0), the chain of `from` from the vehicle at (0, 0) and its waypoints, one call. */
    {
        int8_t cost[81] = {0};
        const pwpp_reach_params reach_params = {1, 100, -1, 0, 0, 0};
        const pwpp_route_params route_params = {0, 8, 64, 0};
        const int32_t goal[2] = {8, 0}, vehicle[2] = {0, 0};
        pwpp_route route;
        int32_t waypoints[8];
        int y, k;
        for (y = 0; y < 8; ++y) cost[9 * y + 4] = 100;
        if (pwpp_plan_grid(h, 9, 9, 1, PWPP_MEM_HOST, cost, NULL, &reach_params, goal, 1, vehicle, 1, 1, &route_params, &route, NULL, waypoints, NULL, NULL) != PWPP_OK)
            return fail("pwpp_plan_grid");
        printf("route round a wall: status %d, %d cells, cost %d, %d edge and %d corner steps, %d waypoints:", (int)route.status, (int)route.cells, (int)route.cost,
               (int)route.edge_steps, (int)route.corner_steps, (int)route.waypoints);
        for (k = 0; k < route.waypoints && k < 8; ++k) printf(" (%d, %d)", (int)(waypoints[k] % 9), (int)(waypoints[k] / 9));
        printf("\n");
    }

    /* A footprint (pwpp_footprint_grid, no reference counterpart): the same wall; a vehicle of 3 x 1 cells (ticks of 1/16 cell, p on the
     * rear axle) drives along row 2 towards it heading +x, and along column 1 heading +y where nothing stands in its way. */
    {
        int8_t cost[81] = {0};
        const pwpp_reach_params reach_params = {1, 100, -1, 0, 0, 0};
        const pwpp_footprint_params foot = {40, 8, 8, 0, {0, 0}};
        int32_t poses[2][6][4];
        pwpp_footprint_traj_row rows[2];
        int y, k;
        for (y = 0; y < 8; ++y) cost[9 * y + 4] = 100;
        for (k = 0; k < 6; ++k) {
            poses[0][k][0] = 8 + 16 * k, poses[0][k][1] = 40, poses[0][k][2] = 1, poses[0][k][3] = 0;
            poses[1][k][0] = 24, poses[1][k][1] = 8 + 16 * k, poses[1][k][2] = 0, poses[1][k][3] = 1;
        }
        if (pwpp_footprint_grid(h, 9, 9, 1, PWPP_MEM_HOST, cost, NULL, NULL, &reach_params, &foot, &poses[0][0][0], 1, 2, 6, NULL, rows) != PWPP_OK)
            return fail("pwpp_footprint_grid");
        for (k = 0; k < 2; ++k)
            printf("footprint along %s: first hit at step %d, %d free steps, the last one %d\n", k ? "column 1" : "row 2", (int)rows[k].first_hit, (int)rows[k].free_steps,
                   (int)rows[k].last);
    }

    /* An outline (pwpp_hull_points, host only, no reference counterpart; pwpp_hull_obstacles does the same for every cluster of a
     * frame on the device): a car seen from a corner is an L of two walls -- its hull is a triangle and the tightest rectangle
     * stands on a wall, where the box of the principal axis would stand on the diagonal. */
    {
        const pwpp_ground_grid grid = {0.0, 0.0, 0.5, 32, 32, 0, 0};
        float wall[9][3];
        int32_t row[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, vertices[8][2];
        pwpp_obstacle_hull hull;
        double xy[2];
        int k;
        for (k = 0; k < 9; ++k) wall[k][0] = k < 5 ? 2.0f + (float)k : 2.0f, wall[k][1] = k < 5 ? 3.0f : 3.0f + 0.5f * (float)(k - 4), wall[k][2] = 0.5f;
        if (pwpp_hull_points(&grid, &wall[0][0], row, 9, &hull, 1, &vertices[0][0], 8) != PWPP_OK) return fail("pwpp_hull_points");
        if (pwpp_hull_vertex_xy(&grid, vertices[0], xy) != PWPP_OK) return fail("pwpp_hull_vertex_xy");
        printf("outline of an L: %d points, %d vertices from (%.1f, %.1f), rectangle %.1f x %.1f m on edge %d, heading (%.0f, %.0f)\n", (int)hull.points,
               (int)hull.n_vertices, xy[0], xy[1], (double)hull.length, (double)hull.width, (int)hull.rect_edge, (double)hull.ax, (double)hull.ay);
    }
    pwpp_destroy(h);

    /* A tilted sensor (pwpp_set_input_transforms, no reference counterpart): the same frame as a LiDAR pitched by 5 degrees and
     * mounted 0.2 m higher would deliver it, and the matrix [R | t] that levels it again handed to the library, which applies it
     * while it bins the points -- no transformed copy of the cloud.  pwpp_transform_points (host only) is the same arithmetic: here
     * it builds the tilted cloud with the inverse map; a caller uses it to carry positions into the levelled frame. */
    {
        const float c5 = 0.9961947f, s5 = 0.08715574f;  /* cos, sin of 5 degrees */
        const float level[12] = {c5, 0.0f, s5, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, -s5, 0.0f, c5, 0.2f};     /* Ry(5 deg), then up 0.2 m */
        const float tilt[12] = {c5, 0.0f, -s5, 0.2f * s5, 0.0f, 1.0f, 0.0f, 0.0f, s5, 0.0f, c5, -0.2f * c5}; /* its inverse */
        float *xyz = (float *)malloc((size_t)n * 3 * sizeof(float)), *tilted = (float *)malloc((size_t)n * 4 * sizeof(float));
        pwpp_handle *h2 = NULL;
        int32_t g2 = 0, ng2 = 0, np2 = 0;
        int i;
        if (!xyz || !tilted) return 1;
        for (i = 0; i < n; ++i) {
            xyz[3 * i] = pts[4 * i];
            xyz[3 * i + 1] = pts[4 * i + 1];
            xyz[3 * i + 2] = pts[4 * i + 2];
        }
        if (pwpp_transform_points(tilt, xyz, n, xyz) != PWPP_OK) return fail("pwpp_transform_points");
        for (i = 0; i < n; ++i) {
            tilted[4 * i] = xyz[3 * i];
            tilted[4 * i + 1] = xyz[3 * i + 1];
            tilted[4 * i + 2] = xyz[3 * i + 2];
            tilted[4 * i + 3] = pts[4 * i + 3];
        }
        if (pwpp_create(&params, 0, &h2) != PWPP_OK) return fail("pwpp_create");
        if (pwpp_set_input_transforms(h2, level, 1) != PWPP_OK) return fail("pwpp_set_input_transforms");
        if (pwpp_estimate_ground(h2, tilted, n, 4, PWPP_LAYOUT_ROW_MAJOR) != PWPP_OK) return fail("pwpp_estimate_ground (tilted)");
        if (pwpp_get_counts(h2, 0, &g2, &ng2, &np2) != PWPP_OK) return fail("pwpp_get_counts");
        printf("tilted sensor, levelled while binning: ground %d nonground %d patches %d (level frame: %d / %d / %d)\n", (int)g2, (int)ng2,
               (int)np2, (int)n_ground, (int)n_nonground, (int)n_patches);
        pwpp_destroy(h2);
        free(xyz);
        free(tilted);
    }

    /* Batches in flight (pwpp_pipe_*, no reference counterpart): four batches of three independent frames through a pipe of depth 2.
     * From pageable host memory a submit returns with the batch done (PWPP_MEM_HOST); device or pinned buffers make it asynchronous
     * and the two handles overlap.  The handle a submit returns holds that batch until it comes round again -- and belongs to the
     * pipe: it is gone after pwpp_pipe_destroy. */
    {
        pwpp_pipe *pipe = NULL;
        const float *frames[3];
        int32_t ns[3];
        int k, same = 1, bad = 0;
        frames[0] = frames[1] = frames[2] = pts;
        ns[0] = ns[1] = ns[2] = n;
        if (pwpp_pipe_create(&params, 0, 2, &pipe) != PWPP_OK) return fail("pwpp_pipe_create");
        for (k = 0; k < 4 && !bad; ++k) {
            pwpp_handle *holder = NULL;
            int32_t g = 0, ng = 0, np = 0;
            int fr;
            if (pwpp_pipe_submit(pipe, frames, ns, 3, 4, PWPP_LAYOUT_ROW_MAJOR, PWPP_MEM_HOST, PWPP_MODE_FRESH, &holder) != PWPP_OK) bad = fail("pwpp_pipe_submit");
            if (!bad && pwpp_synchronize(holder) != PWPP_OK) bad = fail("pwpp_synchronize");
            if (!bad && holder != pwpp_pipe_handle(pipe, k % 2)) same = 0;
            for (fr = 0; fr < 3 && !bad; ++fr) {
                if (pwpp_get_counts(holder, fr, &g, &ng, &np) != PWPP_OK) bad = fail("pwpp_get_counts");
                if (g != n_ground || ng != n_nonground || np != n_patches) same = 0;
            }
        }
        if (!bad && pwpp_pipe_drain(pipe) != PWPP_OK) bad = fail("pwpp_pipe_drain");
        if (!bad) printf("pipe depth 2: 4 batches of 3 frames, every frame %s the single call\n", same ? "equal to" : "DIFFERENT FROM");

        /* The same pipe in PWPP_MODE_STREAMS (the reference's real use, demo_sequential.cpp:54-67: one long-lived object per sensor):
         * two GROUPS of two stateful streams, handle g owns group g, submit k carries the next frame of every stream of group k mod 2.
         * Every stream sees the same frame three times, so all four must end at the sensor height one handle reaches on its own. */
        if (!bad) {
            pwpp_handle *one = NULL;
            double want = 0.0;
            int step, ok = 1;
            if (pwpp_create(&params, 0, &one) != PWPP_OK) bad = fail("pwpp_create");
            for (step = 0; step < 3 && !bad; ++step)
                if (pwpp_estimate_ground(one, pts, n, 4, PWPP_LAYOUT_ROW_MAJOR) != PWPP_OK) bad = fail("pwpp_estimate_ground");
            if (!bad) want = pwpp_get_height(one);
            pwpp_destroy(one);
            if (!bad && pwpp_pipe_set_num_streams(pipe, 2) != PWPP_OK) bad = fail("pwpp_pipe_set_num_streams");
            for (k = 0; k < 6 && !bad; ++k)  /* three steps of each of the two groups */
                if (pwpp_pipe_submit(pipe, frames, ns, 2, 4, PWPP_LAYOUT_ROW_MAJOR, PWPP_MEM_HOST, PWPP_MODE_STREAMS, NULL) != PWPP_OK) bad = fail("pwpp_pipe_submit (streams)");
            if (!bad && pwpp_pipe_drain(pipe) != PWPP_OK) bad = fail("pwpp_pipe_drain");
            for (k = 0; k < 2 && !bad; ++k) {
                pwpp_state st[2];
                if (pwpp_get_state(pwpp_pipe_handle(pipe, k), 0, &st[0]) != PWPP_OK || pwpp_get_state(pwpp_pipe_handle(pipe, k), 1, &st[1]) != PWPP_OK) bad = fail("pwpp_get_state");
                else if (st[0].sensor_height != want || st[1].sensor_height != want) ok = 0;
            }
            if (!bad) printf("pipe in stream mode: 2 groups of 2 streams, 3 steps each, every stream %s one handle's sensor height %.6f\n", ok ? "at" : "AWAY FROM", want);
        }
        pwpp_pipe_destroy(pipe); /* (also on the error paths above: the pipe owns two handles and their workspaces) */
        if (bad) {
            free(pts);
            return bad;
        }
    }
    free(pts);
    return 0;
}
