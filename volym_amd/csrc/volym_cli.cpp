// volym [run simple | benchmark] [-d] -- headless counterpart of the reference binary
// (src/cli.rs:4-56, src/main.rs:42-49).  See volym_amd/__main__.py for the Python twin.
//
//   benchmark : the reference's sweep (src/main.rs:178-345): 4 step sizes x {Base, Importance x {10,15,20},
//               ImportanceCone x {10,15,20}} = 28 rows, 3 trials, 1024x768; benchmark_results.csv with the
//               reference's columns (src/main.rs:71-85) + Mrays/s, algorithmic bytes, GB/s, roofline fraction.
//               A trial is --secs of back-to-back compute passes timed with HIP events (the reference counts
//               presented frames over 2 s of wall clock, blit/GUI/vsync included).
//   run simple: one frame of the interactive default view (src/state.rs:41-55) to frame.ppm; --slice AXIS,INDEX also writes the
//   slice normal to x, y or z through that texel (Simple::slice) to frame_slice_<axis>.ppm; --project MAX|MEAN[,STEP] the
//   maximum or mean intensity projection of the view (Simple::project) to frame_project_<mode>.ppm; --measure [NAME,...] prints
//   the table of segment statistics of the scene in view (Simple::measure); --surface [NAME,...][:MIN_BYTE] prints the surface
//   table (Simple::surface) and --surface-out FILE.stl writes the mesh of those segments together; --components [NAME,...][:MIN_BYTE]
//   prints each segment's connected pieces: how many, the largest, and the ten largest with root and box (Simple::components);
//   --distance [NAME,...][:MIN_BYTE] prints the distance map's summary for the union of those segments -- solid texels, the deepest
//   point, the nearest texel of every segment -- and --distance-inside measures inside the set instead (Simple::distance).
//   --relabel FROM[,FROM...]:TO relabels those segments on the device before the picture (Simple::relabel) and prints what changed;
//   --labels-out FILE writes the labels as they stand afterwards, raw bytes in the orientation of --labels;
//   --brush X,Y,Z[/X,Y,Z...]:TO:R2 paints label TO within sqrt(R2) texels of that polyline of texels (Simple::brush), after --relabel;
//   --lasso X,Y/X,Y/X,Y[/...]:FROM[,FROM...]:TO cuts with the scissors: the texels of the segments FROM under that polygon of pixels of
//   the first frame join TO (Simple::lasso), after --brush;
//   --smooth [NAME,...][:R[,R,R]] smooths the segmentation: one pass of the majority filter over R texels (default 1) for the segments
//   NAME against label 0, or jointly for every label without a name (Simple::smooth), after --lasso;
//   --flood [NAME,...][:R] grows the segments NAME (none: every segment) at once THROUGH the unlabelled matter of density above 0: a
//   texel joins the segment whose seed is the fewest 6-connected steps away, at most R steps (Simple::flood), after --fill;
//   --grow-from-seeds NAME[,NAME...][:CONTRAST[:MAX_COST]] grows the segments NAME at once through the unlabelled matter of density
//   above 0, a step costing 1 and CONTRAST (default 16) per byte of density change across it: a texel joins the segment that reaches
//   it most cheaply, for at most MAX_COST (Simple::grow_from_seeds), after --flood;
//   --fill-between NAME[,NAME...]:AXIS[:MAX_GAP] interpolates each segment NAME, painted on some slices perpendicular to AXIS (x, y or z),
//   across the slices between them; gaps of more than MAX_GAP slices are left alone (Simple::fill_between), after --grow-from-seeds;
//   --fill [NAME,...][:R] grows the segments NAME (none: every segment) at once into the unlabelled matter: every unlabelled texel
//   with a density byte above 0 joins the segment it is nearest to, at most R texels away (Simple::fill), after --smooth;
//   --undo N keeps a history of the edits on the device (Simple::history) and takes the last N back before both, printing each.
#include <algorithm>
#include <cctype>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "demo.hpp"

using namespace volym;

namespace {

std::vector<uint8_t> read_file(const std::string& path)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) throw Error(VOLYM_E_INVALID, "cannot read " + path);
    return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), {});
}

struct Options {
    std::string command = "run";
    std::string volume, labels, segments, output = "benchmark_results.csv";
    uint32_t width = 0, height = 0;
    double secs = 0.25;
    int device = 0;
    int frames_in_flight = 1;      // 2: VOLYM_OPT_FRAMES_IN_FLIGHT (benchmark: frames per wall clock)
    bool debug = false;
    bool crop = false;             // --crop x0,y0,z0,x1,y1,z1: crop box in unit-cube coordinates (run simple)
    float crop_lo[3] = {0.0f, 0.0f, 0.0f}, crop_hi[3] = {1.0f, 1.0f, 1.0f};
    bool clip = false;             // --clip-plane nx,ny,nz,px,py,pz: clip plane in unit-cube coordinates (run simple)
    float clip_normal[3] = {0.0f, 0.0f, 0.0f}, clip_point[3] = {0.5f, 0.5f, 0.5f};
    std::vector<uint8_t> hide;     // --hide 3,4: label values of the segments to hide (run simple)
    int slice_axis = -1;           // --slice z,128: also write the slice normal to that axis through that texel (run simple)
    uint32_t slice_index = 0;
    int project_mode = -1;         // --project MAX|MEAN[,STEP]: also write the projection view (run simple)
    float project_step = 0.0f;     // 0: the march's dense step
    bool measure = false;          // --measure [NAME,...]: also print the table of segment statistics (run simple)
    std::vector<std::string> measure_names;
    std::vector<std::string> relabel_from;   // --relabel FROM[,FROM...]:TO: relabel segments on the device before the picture (run simple)
    std::string relabel_to;
    std::vector<std::array<uint32_t, 3>> brush_points;   // --brush X,Y,Z[/X,Y,Z...]:TO:R2: one stroke of the brush in texel coordinates (run simple)
    std::string brush_to;
    uint32_t brush_r2 = 0;
    std::vector<std::array<int32_t, 2>> lasso_pixels;    // --lasso X,Y/X,Y/X,Y[/...]:FROM[,FROM...]:TO: the scissors over a polygon of pixels (run simple)
    std::vector<std::string> lasso_from;
    std::string lasso_to;
    bool smooth = false;                                 // --smooth [NAME,...][:R[,R,R]]: one pass of the majority filter (run simple)
    std::vector<std::string> smooth_names;
    std::array<uint32_t, 3> smooth_radius = {1u, 1u, 1u};
    bool fill = false;                                   // --fill [NAME,...][:R]: the segments grow at once into the unlabelled matter (run simple)
    std::vector<std::string> fill_names;
    double fill_r = -1.0;                                // (below 0: however far)
    bool flood = false;                                  // --flood [NAME,...][:R]: the segments grow at once through the unlabelled matter (run simple)
    std::vector<std::string> flood_names;
    double flood_r = -1.0;                               // (below 0: however far)
    bool grow = false;                                   // --grow-from-seeds NAME[,NAME...][:CONTRAST[:MAX_COST]]: the segments grow by cost (run simple)
    std::vector<std::string> grow_names;
    uint32_t grow_contrast = 16u, grow_max_cost = 0u;    // (0: however much)
    bool between = false;                                // --fill-between NAME[,NAME...]:AXIS[:MAX_GAP]: the segments are interpolated across gaps (run simple)
    std::vector<std::string> between_names;
    uint32_t between_axis = 2u, between_max_gap = 0u;    // (0: no limit)
    uint32_t undo = 0;             // --undo N: keep a history of the label edits on the device and take the last N back (run simple)
    std::string labels_out;        // --labels-out FILE: the labels as they stand after the edits, raw bytes (run simple)
    bool surface = false;          // --surface [NAME,...][:MIN_BYTE]: also print the surface table (run simple)
    std::vector<std::string> surface_names;
    uint32_t surface_min_byte = 1;
    bool components = false;       // --components [NAME,...][:MIN_BYTE]: also print each segment's connected pieces (run simple)
    std::vector<std::string> components_names;
    uint32_t components_min_byte = 1u;
    std::string surface_out;       // --surface-out FILE.stl: also write the mesh of those segments together
    bool distance = false;         // --distance [NAME,...][:MIN_BYTE]: also print the distance map's summary (run simple)
    bool distance_inside = false;  // --distance-inside: distances inside the set, to its complement
    std::vector<std::string> distance_names;
    uint32_t distance_min_byte = 1u;
};

SimpleAssets load_assets(const Options& o, std::string& what)
{
    SimpleAssets a;
    if (!o.volume.empty()) {
        a.volume_raw = read_file(o.volume);
        if (!o.labels.empty()) a.labels_raw = read_file(o.labels);
        if (!o.segments.empty()) {
            const std::vector<uint8_t> j = read_file(o.segments);
            if (!parse_segments_json(std::string(j.begin(), j.end()), a.segments)) throw Error(VOLYM_E_INVALID, "bad segments JSON");
        }
        what = "file:" + o.volume;
        return a;
    }
    // the reference's default dataset is not distributed (.MISSING_LARGE_BLOBS): synthetic stand-in
    const uint32_t nx = 256, ny = 256, nz = 178;
    a.volume_raw.resize(static_cast<size_t>(nx) * ny * nz);
    a.labels_raw.resize(a.volume_raw.size());
    volym_synth_teapot(nx, ny, nz, 20250310u, a.volume_raw.data(), a.labels_raw.data());
    a.segments = {{"Segment_4", "Cup", 1, 3, 0}, {"Segment_5", "Ground", 2, 4, 0}, {"Segment_2", "Lobster", 0, 2, 255}};
    what = "synthetic teapot 256x256x178";
    return a;
}

void mean_std(const std::vector<double>& v, double& m, double& s)
{
    m = 0; for (double x : v) m += x; m /= v.size();
    s = 0; for (double x : v) s += (x - m) * (x - m); s = std::sqrt(s / v.size());   // population, src/main.rs:124-158
}

int benchmark_all(const Options& o)
{
    const uint32_t W = o.width ? o.width : 1024, H = o.height ? o.height : 768;       // src/main.rs:356-359
    std::string what;
    const SimpleAssets assets = load_assets(o, what);
    const float step_sizes[] = {0.0030f, 0.0050f, 0.0100f, 0.0200f};                  // src/main.rs:192
    const uint32_t importance_steps[] = {10, 15, 20};                                  // src/main.rs:193
    const int NUM_TRIALS = 3;                                                          // src/main.rs:179
    struct Row { const char* algo; float step; uint32_t isteps; bool cone; };
    std::vector<Row> rows;
    for (float s : step_sizes) rows.push_back({"Base", s, 0, false});
    for (float s : step_sizes) for (uint32_t n : importance_steps) rows.push_back({"Importance", s, n, false});
    for (float s : step_sizes) for (uint32_t n : importance_steps) rows.push_back({"ImportanceCone", s, n, true});

    std::printf("volym benchmark: %s, %ux%u, %zu rows x %d trials of %.2f s\n", what.c_str(), W, H, rows.size(), NUM_TRIALS, o.secs);
    GpuContext ctx(W, H, o.device);
    if (o.frames_in_flight == 2) ctx.check(volym_set_option(ctx.handle(), VOLYM_OPT_FRAMES_IN_FLIGHT, 2));   // before the scene
    // total milliseconds of n frames: per-launch HIP events on one stream, or -- two frames in flight -- the wall clock of n compute
    // passes enqueued back to back (the reference counts presented frames over wall time, src/main.rs:113-135)
    auto trial = [&](uint32_t n, std::vector<float>& ms) -> double {
        if (o.frames_in_flight != 2) {
            ms.assign(n, 0.0f);
            ctx.check(volym_time_passes(ctx.handle(), n, ms.data()));
            double total = 0; for (float x : ms) total += x;
            return total;
        }
        ctx.check(volym_sync(ctx.handle()));
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t i = 0; i < n; ++i) ctx.check(volym_compute_pass(ctx.handle()));
        ctx.check(volym_sync(ctx.handle()));
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    };
    const StateParameters base = StateParameters::benchmark();                        // src/main.rs:180-190
    State state = State::with_parameters(static_cast<float>(W) / static_cast<float>(H), base);
    Simple demo = Simple::init(ctx, state, assets);
    std::ofstream csv(o.output);
    csv << "algorithm,step_size,importance_steps,use_cone,avg_total_frames,avg_total_time_ms,avg_frame_time_ms,avg_fps,"
           "std_dev_total_frames,std_dev_total_time_ms,std_dev_frame_time_ms,std_dev_fps,"
           "mrays_per_s,b_alg_bytes_per_frame,algorithmic_gb_per_s,hbm_roofline_fraction,n_gpus\n";
    for (const Row& r : rows) {
        StateParameters p = base;
        p.raymarching_step_size = r.step;
        if (std::strcmp(r.algo, "Base") != 0) {
            p.use_importance_rendering = 1; p.importance_check_ahead_steps = r.isteps; p.use_cone_importance_check = r.cone ? 1 : 0;
        }
        state = State::with_parameters(static_cast<float>(W) / static_cast<float>(H), p);
        state.update();                                                               // src/event_loop.rs:100
        demo.update_gpu_state(ctx, state);
        std::vector<float> ms(8);
        ctx.check(volym_time_passes(ctx.handle(), 8, ms.data()));
        std::sort(ms.begin(), ms.end());
        const double per = std::max<double>(ms[4], 1e-3);
        const uint32_t n = static_cast<uint32_t>(std::min(std::max(o.secs * 1e3 / per, 4.0), 20000.0));
        std::vector<double> frames, times, ftimes, fps;
        if (o.frames_in_flight == 2) { trial(8, ms); ctx.check(volym_settle(ctx.handle())); }   // both frame contexts warm, their lists in place
        for (int t = 0; t < NUM_TRIALS; ++t) {
            const double total = trial(n, ms);
            frames.push_back(n); times.push_back(total); ftimes.push_back(total / n); fps.push_back(n / (total * 1e-3));
        }
        volym_stats st;
        ctx.check(volym_stats_pass(ctx.handle(), &st));
        const double b_alg = static_cast<double>(st.n_vol) + st.n_imp + 4.0 * W * H;
        double m[4], s[4];
        mean_std(frames, m[0], s[0]); mean_std(times, m[1], s[1]); mean_std(ftimes, m[2], s[2]); mean_std(fps, m[3], s[3]);
        const double mrays = W * static_cast<double>(H) / (m[2] * 1e-3) / 1e6, gbs = b_alg / (m[2] * 1e-3) / 1e9;
        csv << r.algo << ',' << r.step << ',' << r.isteps << ',' << (r.cone ? "true" : "false");
        for (double v : m) csv << ',' << v;
        for (double v : s) csv << ',' << v;
        csv << ',' << mrays << ',' << static_cast<unsigned long long>(b_alg) << ',' << gbs << ',' << gbs / 8000.0 << ",1\n";
        std::printf("%-14s step %.4f steps %2u: %8.3f ms/frame %9.1f fps %9.0f Mrays/s  B_alg %6.1f MB  %5.1f%% of HBM roofline\n", r.algo,
                    r.step, r.isteps, m[2], m[3], mrays, b_alg / 1e6, 100.0 * gbs / 8000.0);
        std::fflush(stdout);
    }
    std::printf("wrote %s\n", o.output.c_str());
    return 0;
}

int run_simple(const Options& o)
{
    const uint32_t W = o.width ? o.width : 1280, H = o.height ? o.height : 720;
    std::string what;
    const SimpleAssets assets = load_assets(o, what);
    GpuContext ctx(W, H, o.device);
    State state = State::with_parameters(static_cast<float>(W) / static_cast<float>(H), StateParameters());   // src/state.rs:41-55
    state.update();
    Simple demo = Simple::init(ctx, state, assets);
    if (o.crop) demo.set_crop(ctx, assets, o.crop_lo, o.crop_hi);
    if (o.clip) demo.set_clip_plane(ctx, assets, o.clip_normal, o.clip_point);
    if (!o.hide.empty()) demo.set_hidden(ctx, assets, o.hide);
    if (o.undo != 0u) demo.history(ctx, assets);                  // on before the edits: a step is journalled by the edit it takes back
    volym_relabel_result relabelled{};
    if (!o.relabel_to.empty()) relabelled = demo.relabel(ctx, assets, o.relabel_from, o.relabel_to);
    volym_relabel_result brushed{};
    if (!o.brush_to.empty()) brushed = demo.brush(ctx, assets, o.brush_points, o.brush_to, o.brush_r2);       // after --relabel, before --undo
    volym_relabel_result lassoed{};
    if (!o.lasso_to.empty()) lassoed = demo.lasso(ctx, assets, o.lasso_pixels, o.lasso_from, o.lasso_to);   // the view of the first frame; after --brush, before --undo
    volym_relabel_result smoothed{};
    if (o.smooth) smoothed = demo.smooth(ctx, assets, o.smooth_names, o.smooth_radius);                     // after --lasso, before --undo
    volym_relabel_result filled{};
    if (o.fill) filled = demo.fill(ctx, assets, o.fill_names, o.fill_r);                                    // after --smooth, before --undo
    volym_relabel_result flooded{};
    if (o.flood) flooded = demo.flood(ctx, assets, o.flood_names, o.flood_r);                               // after --fill, before --undo
    volym_relabel_result grown{};
    if (o.grow) grown = demo.grow_from_seeds(ctx, assets, o.grow_names, o.grow_contrast, o.grow_max_cost);   // after --flood, before --undo
    std::vector<Simple::FilledBetween> between;
    if (o.between) between = demo.fill_between(ctx, assets, o.between_names, o.between_axis, o.between_max_gap);   // after --grow-from-seeds, before --undo
    std::vector<std::pair<bool, volym_relabel_result>> undone(o.undo);       // the last N edits back, before the picture and --labels-out
    for (auto& u : undone) u.first = demo.undo(ctx, u.second);
    demo.update_gpu_state(ctx, state);
    demo.compute_pass(ctx);
    ctx.check(volym_sync(ctx.handle()));
    std::vector<uint8_t> rgba(static_cast<size_t>(W) * H * 4);
    ctx.check(volym_read_rgba8(ctx.handle(), rgba.data()));
    const std::string path = o.output == "benchmark_results.csv" ? "frame.ppm" : o.output;
    std::ofstream f(path, std::ios::binary);
    f << "P6\n" << W << ' ' << H << "\n255\n";
    for (size_t i = 0; i < static_cast<size_t>(W) * H; ++i) f.write(reinterpret_cast<const char*>(&rgba[4 * i]), 3);
    std::printf("run simple: %s, %ux%u -> %s\n", what.c_str(), W, H, path.c_str());
    const auto print_result = [](const char* what, const volym_relabel_result& r) {
        std::printf("%s: %llu texels changed", what, static_cast<unsigned long long>(r.changed));
        if (r.changed != 0u) std::printf(", box [%u,%u,%u)..[%u,%u,%u)", r.box[0], r.box[1], r.box[2], r.box[3], r.box[4], r.box[5]);
        for (int l = 0; l < 256; ++l)
            if (r.left[l] != 0u || r.arrived[l] != 0u)
                std::printf("; label %d: -%llu +%llu", l, static_cast<unsigned long long>(r.left[l]), static_cast<unsigned long long>(r.arrived[l]));
        std::printf("\n");
    };
    if (!o.relabel_to.empty()) print_result("relabel", relabelled);
    if (!o.brush_to.empty()) print_result("brush", brushed);
    if (!o.lasso_to.empty()) print_result("lasso", lassoed);
    if (o.smooth) print_result("smooth", smoothed);
    if (o.fill) {
        // how many texels joined the nearest segment, then every segment that took some
        int took = 0;
        for (int l = 0; l < 256; ++l) took += filled.arrived[l] != 0u;
        std::printf("fill: %llu texels joined the nearest of %d segments\n", static_cast<unsigned long long>(filled.changed), took);
        for (int l = 0; l < 256; ++l) {
            if (filled.arrived[l] == 0u) continue;
            std::string name = "label " + std::to_string(l);
            for (const SegmentInfo& s : assets.segments) if (s.label_value == l) name = s.name.empty() ? s.id : s.name;
            std::printf("  + %-16s label %3d: %10llu\n", name.c_str(), l, static_cast<unsigned long long>(filled.arrived[l]));
        }
    }
    if (o.flood) {
        // how many texels joined a segment through the matter, then every segment that took some
        int took = 0;
        for (int l = 0; l < 256; ++l) took += flooded.arrived[l] != 0u;
        std::printf("flood: %llu texels joined %d segments through the matter\n", static_cast<unsigned long long>(flooded.changed), took);
        for (int l = 0; l < 256; ++l) {
            if (flooded.arrived[l] == 0u) continue;
            std::string name = "label " + std::to_string(l);
            for (const SegmentInfo& s : assets.segments) if (s.label_value == l) name = s.name.empty() ? s.id : s.name;
            std::printf("  + %-16s label %3d: %10llu\n", name.c_str(), l, static_cast<unsigned long long>(flooded.arrived[l]));
        }
    }
    if (o.grow) {
        // how many texels joined the segment that reaches them most cheaply, then every segment that took some
        int took = 0;
        for (int l = 0; l < 256; ++l) took += grown.arrived[l] != 0u;
        std::printf("grow from seeds: %llu texels joined the cheapest of %d segments\n", static_cast<unsigned long long>(grown.changed), took);
        for (int l = 0; l < 256; ++l) {
            if (grown.arrived[l] == 0u) continue;
            std::string name = "label " + std::to_string(l);
            for (const SegmentInfo& s : assets.segments) if (s.label_value == l) name = s.name.empty() ? s.id : s.name;
            std::printf("  + %-16s label %3d: %10llu\n", name.c_str(), l, static_cast<unsigned long long>(grown.arrived[l]));
        }
    }
    for (const auto& f : between) {
        // per segment the keys, the gaps filled and refused and the texels that joined and left
        std::string name = "label " + std::to_string(f.label);
        for (const SegmentInfo& s : assets.segments) if (s.label_value == static_cast<int>(f.label)) name = s.name.empty() ? s.id : s.name;
        std::printf("fill between: %s label %u, %u key slices, %u gaps of %u slices filled, %u refused: %llu texels joined, %llu left\n", name.c_str(), f.label, f.n_keys,
                    f.n_gaps, f.n_gap_slices, f.n_refused, static_cast<unsigned long long>(f.result.arrived[f.label]),
                    static_cast<unsigned long long>(f.result.left[f.label]));
    }
    for (const auto& u : undone) {
        if (u.first) print_result("undo", u.second);
        else std::printf("undo: nothing to take back\n");
    }
    if (!o.labels_out.empty()) {
        const std::vector<uint8_t> raw = demo.labels_from_device(ctx, assets);
        std::ofstream lf(o.labels_out, std::ios::binary);
        lf.write(reinterpret_cast<const char*>(raw.data()), static_cast<std::streamsize>(raw.size()));
        std::printf("labels: %zu bytes -> %s\n", raw.size(), o.labels_out.c_str());
    }
    if (o.slice_axis >= 0) {
        // the slice view beside the frame: transfer-function colours, segments overlaid, cut texels tinted
        SliceView view;
        view.mode = VOLYM_SLICE_TF;
        const volym_slice s = demo.slice(ctx, assets, o.slice_axis, o.slice_index, view);
        std::vector<uint8_t> img(static_cast<size_t>(s.width) * s.height * 4);
        ctx.check(volym_read_slice(ctx.handle(), img.data()));
        const size_t dot = path.rfind('.');
        const std::string stem = dot == std::string::npos ? path : path.substr(0, dot), ext = dot == std::string::npos ? std::string(".ppm") : path.substr(dot);
        const std::string spath = stem + "_slice_" + "xyz"[o.slice_axis] + ext;
        std::ofstream sf(spath, std::ios::binary);
        sf << "P6\n" << s.width << ' ' << s.height << "\n255\n";
        for (size_t i = 0; i < static_cast<size_t>(s.width) * s.height; ++i) sf.write(reinterpret_cast<const char*>(&img[4 * i]), 3);
        std::printf("slice %c: %ux%u -> %s\n", "xyz"[o.slice_axis], s.width, s.height, spath.c_str());
    }
    if (o.project_mode >= 0) {
        // the projection view of the same camera: transfer-function colours, over MAX the brightest sample's segment
        ProjectView view;
        view.step = o.project_step;
        view.tf = true;
        demo.project(ctx, assets, static_cast<uint32_t>(o.project_mode), view);
        std::vector<uint8_t> img(static_cast<size_t>(W) * H * 4);
        ctx.check(volym_read_projection_image(ctx.handle(), img.data()));
        const size_t dot = path.rfind('.');
        const std::string stem = dot == std::string::npos ? path : path.substr(0, dot), ext = dot == std::string::npos ? std::string(".ppm") : path.substr(dot);
        const char* mode = o.project_mode == VOLYM_PROJECT_MEAN ? "mean" : "max";
        const std::string ppath = stem + "_project_" + mode + ext;
        std::ofstream pf(ppath, std::ios::binary);
        pf << "P6\n" << W << ' ' << H << "\n255\n";
        for (size_t i = 0; i < static_cast<size_t>(W) * H; ++i) pf.write(reinterpret_cast<const char*>(&img[4 * i]), 3);
        std::printf("project %s: %ux%u -> %s\n", mode, W, H, ppath.c_str());
    }
    if (o.measure) {
        // what is in view, per segment: the scene under the cuts of this run
        const std::vector<Simple::Measured> rows = demo.measure(ctx, assets, o.measure_names);
        std::printf("%-16s %5s %12s %8s %8s %8s %4s %4s  %-22s %s\n", "segment", "label", "texels", "in view", "mean", "std", "min", "max", "centroid", "box");
        for (const Simple::Measured& r : rows) {
            if (r.stats.count == 0u) { std::printf("%-16s %5u %12s\n", r.segment.c_str(), r.label, "-"); continue; }
            std::printf("%-16s %5u %12llu %7.1f%% %8.2f %8.2f %4u %4u  (%6.1f,%6.1f,%6.1f) [%d,%d,%d]..[%d,%d,%d]\n", r.segment.c_str(), r.label,
                        static_cast<unsigned long long>(r.stats.count), 100.0 * r.in_view, r.mean, r.std_dev, r.stats.min, r.stats.max, r.centroid[0], r.centroid[1],
                        r.centroid[2], r.stats.box[0], r.stats.box[1], r.stats.box[2], r.stats.box[3], r.stats.box[4], r.stats.box[5]);
        }
    }
    if (o.surface || !o.surface_out.empty()) {
        // the surface of each segment in view, selected alone; the file holds the boundary of all of them together
        const std::vector<Simple::Surfaced> rows = demo.surface(ctx, assets, o.surface_names, o.surface_min_byte);
        std::printf("%-16s %5s %10s %10s %10s %12s %12s %12s %10s\n", "segment", "label", "faces x", "faces y", "faces z", "area", "enclosed", "measured", "sphericity");
        for (const Simple::Surfaced& r : rows)
            std::printf("%-16s %5u %10llu %10llu %10llu %12.1f %12llu %12llu %10.3f\n", r.segment.c_str(), r.label, static_cast<unsigned long long>(r.pairs[0]),
                        static_cast<unsigned long long>(r.pairs[1]), static_cast<unsigned long long>(r.pairs[2]), r.area, static_cast<unsigned long long>(r.enclosed),
                        static_cast<unsigned long long>(r.measured), r.sphericity);
        if (!o.surface_out.empty()) {
            const std::vector<struct volym_surface_face> faces = demo.surface_faces(ctx, assets, o.surface_names, o.surface_min_byte);
            Simple::write_stl(o.surface_out, faces);
            std::printf("surface: %zu faces -> %s\n", faces.size(), o.surface_out.c_str());
        }
    }
    if (o.components) {
        // is each segment one piece: per segment in view, selected alone, its pieces and the ten largest with root and box
        const std::vector<Simple::Pieces> rows = demo.components(ctx, assets, o.components_names, o.components_min_byte);
        if (rows.empty()) std::printf("components: no solid texel\n");
        for (const Simple::Pieces& r : rows) {
            const uint32_t largest = r.top.empty() ? 0u : r.top.front().record.count;
            std::printf("%-16s label %3u: %llu piece%s in %llu solid texels, largest %u texels (%.1f%%), %llu smaller than 8 texels\n", r.segment.c_str(), r.label,
                        static_cast<unsigned long long>(r.pieces), r.pieces == 1u ? "" : "s", static_cast<unsigned long long>(r.solid), largest,
                        100.0 * static_cast<double>(largest) / static_cast<double>(r.solid), static_cast<unsigned long long>(r.small));
            for (const Simple::Piece& p : r.top)
                std::printf("  piece %-8u %10u texels  root (%u,%u,%u)  box [%u,%u,%u]..[%u,%u,%u]%s\n", p.number, p.record.count, p.record.x, p.record.y, p.record.z,
                            p.record.box[0], p.record.box[1], p.record.box[2], p.record.box[3], p.record.box[4], p.record.box[5], (p.record.flags & 1u) ? " open" : "");
        }
    }
    if (o.distance) {
        // margins, thickness, clearance: the summary of the distance map of the named segments' union
        const Simple::Distances r = demo.distance(ctx, assets, o.distance_names, o.distance_inside, o.distance_min_byte);
        const char* mode = o.distance_inside ? " (inside)" : "";
        if (!r.finite)
            std::printf("distance: %llu solid texels%s, deepest (none): no texel at a finite distance\n", static_cast<unsigned long long>(r.summary.n_solid), mode);
        else
            std::printf("distance: %llu solid texels%s, deepest (%u,%u,%u) d2 %u = %.3f, %llu texels at a finite distance\n",
                        static_cast<unsigned long long>(r.summary.n_solid), mode, r.summary.max_at[0], r.summary.max_at[1], r.summary.max_at[2], r.summary.max_d2,
                        std::sqrt(static_cast<double>(r.summary.max_d2)), static_cast<unsigned long long>(r.summary.n_finite));
        for (const Simple::Nearest& n : r.nearest)
            std::printf("  nearest %-16s label %3u: d2 %10u = %9.3f at (%u,%u,%u)\n", n.segment.c_str(), n.label, n.d2, std::sqrt(static_cast<double>(n.d2)), n.at[0], n.at[1],
                        n.at[2]);
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    Options o;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto next = [&]() -> std::string { if (i + 1 >= argc) throw Error(VOLYM_E_INVALID, "missing value for " + a); return argv[++i]; };
        try {
            if (a == "run") { o.command = "run"; if (i + 1 < argc && std::string(argv[i + 1]) == "simple") ++i; }
            else if (a == "benchmark") o.command = "benchmark";
            else if (a == "-d" || a == "--debug") o.debug = true;
            else if (a == "--volume") o.volume = next();
            else if (a == "--labels") o.labels = next();
            else if (a == "--segments") o.segments = next();
            else if (a == "--output") o.output = next();
            else if (a == "--width") o.width = static_cast<uint32_t>(std::stoul(next()));
            else if (a == "--height") o.height = static_cast<uint32_t>(std::stoul(next()));
            else if (a == "--secs") o.secs = std::stod(next());
            else if (a == "--device") o.device = std::stoi(next());
            else if (a == "--frames-in-flight") { o.frames_in_flight = std::stoi(next()); if (o.frames_in_flight != 1 && o.frames_in_flight != 2) throw Error(VOLYM_E_INVALID, "--frames-in-flight: 1 or 2"); }
            else if (a == "--crop") {
                const std::string v = next();
                float f[6];
                if (std::sscanf(v.c_str(), "%f,%f,%f,%f,%f,%f", &f[0], &f[1], &f[2], &f[3], &f[4], &f[5]) != 6) throw Error(VOLYM_E_INVALID, "--crop: x0,y0,z0,x1,y1,z1 in [0, 1]");
                for (int k = 0; k < 3; ++k) { o.crop_lo[k] = f[k]; o.crop_hi[k] = f[3 + k]; }
                o.crop = true;
            }
            else if (a == "--clip-plane") {
                const std::string v = next();
                float f[6];
                if (std::sscanf(v.c_str(), "%f,%f,%f,%f,%f,%f", &f[0], &f[1], &f[2], &f[3], &f[4], &f[5]) != 6) throw Error(VOLYM_E_INVALID, "--clip-plane: nx,ny,nz,px,py,pz (normal and point, unit-cube coordinates)");
                for (int k = 0; k < 3; ++k) { o.clip_normal[k] = f[k]; o.clip_point[k] = f[3 + k]; }
                o.clip = true;
            }
            else if (a == "--hide") {
                const std::string v = next();
                size_t pos = 0;
                while (pos <= v.size()) {
                    const size_t comma = std::min(v.find(',', pos), v.size());
                    size_t used = 0;
                    const std::string item = v.substr(pos, comma - pos);
                    int l = -1;
                    try { l = std::stoi(item, &used); } catch (const std::exception&) { used = 0; }
                    if (item.empty() || used != item.size() || l < 0 || l > 255) throw Error(VOLYM_E_INVALID, "--hide: label values 0..255, comma separated");
                    o.hide.push_back(static_cast<uint8_t>(l));
                    pos = comma + 1u;
                }
            }
            else if (a == "--slice") {
                const std::string v = next();
                size_t used = 0;
                unsigned long index = 0;
                const size_t axis = v.size() >= 3 && v[1] == ',' ? std::string("xyz").find(v[0]) : std::string::npos;
                try { index = std::stoul(v.substr(2), &used); } catch (const std::exception&) { used = 0; }
                if (axis == std::string::npos || used == 0 || used != v.size() - 2 || index > 0xffffffffUL) throw Error(VOLYM_E_INVALID, "--slice: AXIS,INDEX -- x, y or z and a texel index along it");
                o.slice_axis = static_cast<int>(axis);
                o.slice_index = static_cast<uint32_t>(index);
            }
            else if (a == "--relabel") {
                const std::string v = next();
                const size_t colon = v.rfind(':');
                if (colon == std::string::npos || colon == 0u || colon + 1u >= v.size()) throw Error(VOLYM_E_INVALID, "--relabel: FROM[,FROM...]:TO -- label values or segment names");
                o.relabel_to = v.substr(colon + 1u);
                size_t pos = 0;
                while (pos < colon) {
                    const size_t comma = std::min(v.find(',', pos), colon);
                    if (comma > pos) o.relabel_from.push_back(v.substr(pos, comma - pos));
                    pos = comma + 1u;
                }
            }
            else if (a == "--brush") {
                const char* usage = "--brush: X,Y,Z[/X,Y,Z...]:TO:R2 -- texels of the stroke, a label value or segment name, the squared radius";
                const std::string v = next();
                const size_t last = v.rfind(':'), first = last == std::string::npos || last == 0u ? std::string::npos : v.rfind(':', last - 1u);
                if (first == std::string::npos || first == 0u || first + 1u >= last || last + 1u >= v.size()) throw Error(VOLYM_E_INVALID, usage);
                o.brush_to = v.substr(first + 1u, last - first - 1u);
                try {
                    size_t used = 0;
                    const unsigned long r2 = std::stoul(v.substr(last + 1u), &used);
                    if (used != v.size() - last - 1u || r2 > 0xffffffffUL) throw Error(VOLYM_E_INVALID, usage);
                    o.brush_r2 = static_cast<uint32_t>(r2);
                    size_t pos = 0;
                    while (pos < first) {
                        const size_t slash = std::min(v.find('/', pos), first);
                        std::array<uint32_t, 3> p{};
                        const std::string one = v.substr(pos, slash - pos);
                        size_t at = 0;
                        for (int k = 0; k < 3; ++k) {
                            if (at >= one.size() || one[at] < '0' || one[at] > '9') throw Error(VOLYM_E_INVALID, usage);
                            const unsigned long c = std::stoul(one.substr(at), &used);
                            if (c > 0xffffUL) throw Error(VOLYM_E_INVALID, usage);
                            p[static_cast<size_t>(k)] = static_cast<uint32_t>(c);
                            at += used;
                            if (k < 2) { if (at >= one.size() || one[at] != ',') throw Error(VOLYM_E_INVALID, usage); ++at; }
                        }
                        if (at != one.size()) throw Error(VOLYM_E_INVALID, usage);
                        o.brush_points.push_back(p);
                        pos = slash + 1u;
                    }
                } catch (const std::logic_error&) { throw Error(VOLYM_E_INVALID, usage); }
                if (o.brush_points.empty() || o.brush_points.size() > VOLYM_BRUSH_MAX_POINTS) throw Error(VOLYM_E_INVALID, usage);
            }
            else if (a == "--lasso") {
                const char* usage = "--lasso: X,Y/X,Y/X,Y[/...]:FROM[,FROM...]:TO -- pixels of the polygon, the segments it cuts and the segment they join";
                const std::string v = next();
                const size_t last = v.rfind(':'), first = last == std::string::npos || last == 0u ? std::string::npos : v.rfind(':', last - 1u);
                if (first == std::string::npos || first == 0u || first + 1u >= last || last + 1u >= v.size()) throw Error(VOLYM_E_INVALID, usage);
                o.lasso_to = v.substr(last + 1u);
                size_t pos = first + 1u;
                while (pos < last) {
                    const size_t comma = std::min(v.find(',', pos), last);
                    if (comma > pos) o.lasso_from.push_back(v.substr(pos, comma - pos));
                    pos = comma + 1u;
                }
                if (o.lasso_from.empty()) throw Error(VOLYM_E_INVALID, usage);
                try {
                    pos = 0;
                    while (pos < first) {
                        const size_t slash = std::min(v.find('/', pos), first);
                        const std::string one = v.substr(pos, slash - pos);
                        const size_t comma = one.find(',');
                        if (comma == std::string::npos || comma == 0u || comma + 1u >= one.size()) throw Error(VOLYM_E_INVALID, usage);
                        size_t used_x = 0, used_y = 0;
                        const long x = std::stol(one.substr(0, comma), &used_x), y = std::stol(one.substr(comma + 1u), &used_y);
                        if (used_x != comma || used_y != one.size() - comma - 1u || std::labs(x) > VOLYM_LASSO_VERTEX_MAX || std::labs(y) > VOLYM_LASSO_VERTEX_MAX)
                            throw Error(VOLYM_E_INVALID, usage);
                        o.lasso_pixels.push_back({static_cast<int32_t>(x), static_cast<int32_t>(y)});
                        pos = slash + 1u;
                    }
                } catch (const std::logic_error&) { throw Error(VOLYM_E_INVALID, usage); }
                if (o.lasso_pixels.size() < 3u || o.lasso_pixels.size() > VOLYM_LASSO_MAX_POINTS) throw Error(VOLYM_E_INVALID, usage);
            }
            else if (a == "--smooth") {
                const char* usage = "--smooth: [NAME,...][:R[,R,R]] -- the segments to smooth against label 0 (none: every label, jointly) and the radius in texels";
                o.smooth = true;
                std::string v;
                if (i + 1 < argc && argv[i + 1][0] != '-' && std::string(argv[i + 1]) != "run" && std::string(argv[i + 1]) != "benchmark") v = next();
                const size_t colon = v.rfind(':');
                const std::string names = colon == std::string::npos ? v : v.substr(0, colon);
                size_t pos = 0;
                while (pos < names.size()) {
                    const size_t comma = std::min(names.find(',', pos), names.size());
                    if (comma > pos) o.smooth_names.push_back(names.substr(pos, comma - pos));
                    pos = comma + 1u;
                }
                if (colon != std::string::npos) {
                    const std::string r = v.substr(colon + 1u);
                    std::vector<uint32_t> radii;
                    try {
                        pos = 0;
                        while (pos <= r.size()) {
                            const size_t comma = std::min(r.find(',', pos), r.size());
                            const std::string one = r.substr(pos, comma - pos);
                            size_t used = 0;
                            if (one.empty() || one[0] < '0' || one[0] > '9') throw Error(VOLYM_E_INVALID, usage);
                            const unsigned long c = std::stoul(one, &used);
                            if (used != one.size() || c > VOLYM_SMOOTH_MAX_RADIUS) throw Error(VOLYM_E_INVALID, usage);
                            radii.push_back(static_cast<uint32_t>(c));
                            pos = comma + 1u;
                        }
                    } catch (const std::logic_error&) { throw Error(VOLYM_E_INVALID, usage); }
                    if (radii.size() == 1u) o.smooth_radius = {radii[0], radii[0], radii[0]};
                    else if (radii.size() == 3u) o.smooth_radius = {radii[0], radii[1], radii[2]};
                    else throw Error(VOLYM_E_INVALID, usage);
                }
            }
            else if (a == "--fill") {
                const char* usage = "--fill: [NAME,...][:R] -- the segments that grow into the unlabelled matter (none: every segment) and how far in texels";
                o.fill = true;
                std::string v;
                if (i + 1 < argc && argv[i + 1][0] != '-' && std::string(argv[i + 1]) != "run" && std::string(argv[i + 1]) != "benchmark") v = next();
                const size_t colon = v.rfind(':');
                const std::string names = colon == std::string::npos ? v : v.substr(0, colon);
                size_t pos = 0;
                while (pos < names.size()) {
                    const size_t comma = std::min(names.find(',', pos), names.size());
                    if (comma > pos) o.fill_names.push_back(names.substr(pos, comma - pos));
                    pos = comma + 1u;
                }
                if (colon != std::string::npos) {
                    try {
                        size_t used = 0;
                        const std::string r = v.substr(colon + 1u);
                        o.fill_r = std::stod(r, &used);
                        if (used != r.size() || !(o.fill_r >= 0.0)) throw Error(VOLYM_E_INVALID, usage);
                    } catch (const std::logic_error&) { throw Error(VOLYM_E_INVALID, usage); }
                }
            }
            else if (a == "--flood") {
                const char* usage = "--flood: [NAME,...][:R] -- the segments that grow through the unlabelled matter (none: every segment) and how many steps";
                o.flood = true;
                std::string v;
                if (i + 1 < argc && argv[i + 1][0] != '-' && std::string(argv[i + 1]) != "run" && std::string(argv[i + 1]) != "benchmark") v = next();
                const size_t colon = v.rfind(':');
                const std::string names = colon == std::string::npos ? v : v.substr(0, colon);
                size_t pos = 0;
                while (pos < names.size()) {
                    const size_t comma = std::min(names.find(',', pos), names.size());
                    if (comma > pos) o.flood_names.push_back(names.substr(pos, comma - pos));
                    pos = comma + 1u;
                }
                if (colon != std::string::npos) {
                    try {
                        size_t used = 0;
                        const std::string r = v.substr(colon + 1u);
                        o.flood_r = std::stod(r, &used);
                        if (used != r.size() || !(o.flood_r >= 1.0)) throw Error(VOLYM_E_INVALID, usage);
                    } catch (const std::logic_error&) { throw Error(VOLYM_E_INVALID, usage); }
                }
            }
            else if (a == "--grow-from-seeds") {
                const char* usage = "--grow-from-seeds: NAME[,NAME...][:CONTRAST[:MAX_COST]] -- the segments that grow, the cost of a byte of density change (0..255) "
                                    "and the most a texel may cost";
                o.grow = true;
                const std::string v = next();
                std::vector<std::string> parts;
                size_t pos = 0;
                while (pos <= v.size()) {
                    const size_t colon = std::min(v.find(':', pos), v.size());
                    parts.push_back(v.substr(pos, colon - pos));
                    pos = colon + 1u;
                }
                if (parts.empty() || parts.size() > 3u) throw Error(VOLYM_E_INVALID, usage);
                pos = 0;
                while (pos < parts[0].size()) {
                    const size_t comma = std::min(parts[0].find(',', pos), parts[0].size());
                    if (comma > pos) o.grow_names.push_back(parts[0].substr(pos, comma - pos));
                    pos = comma + 1u;
                }
                try {
                    size_t used = 0;
                    if (parts.size() > 1u) {
                        const unsigned long c = std::stoul(parts[1], &used);
                        if (used != parts[1].size() || c > 255ul) throw Error(VOLYM_E_INVALID, usage);
                        o.grow_contrast = static_cast<uint32_t>(c);
                    }
                    if (parts.size() > 2u) {
                        const unsigned long m = std::stoul(parts[2], &used);
                        if (used != parts[2].size() || m > VOLYM_COST_MAX) throw Error(VOLYM_E_INVALID, usage);
                        o.grow_max_cost = static_cast<uint32_t>(m);
                    }
                } catch (const std::logic_error&) { throw Error(VOLYM_E_INVALID, usage); }
                if (o.grow_names.empty()) throw Error(VOLYM_E_INVALID, usage);
            }
            else if (a == "--fill-between") {
                const char* usage = "--fill-between: NAME[,NAME...]:AXIS[:MAX_GAP] -- the segments to interpolate, the axis their painted slices are perpendicular to "
                                    "(x, y or z) and the most slices a gap may have";
                o.between = true;
                const std::string v = next();
                std::vector<std::string> parts;
                size_t pos = 0;
                while (pos <= v.size()) {
                    const size_t colon = std::min(v.find(':', pos), v.size());
                    parts.push_back(v.substr(pos, colon - pos));
                    pos = colon + 1u;
                }
                if (parts.size() < 2u || parts.size() > 3u || parts[1].size() != 1u || parts[1][0] < 'x' || parts[1][0] > 'z') throw Error(VOLYM_E_INVALID, usage);
                o.between_axis = static_cast<uint32_t>(parts[1][0] - 'x');
                pos = 0;
                while (pos < parts[0].size()) {
                    const size_t comma = std::min(parts[0].find(',', pos), parts[0].size());
                    if (comma > pos) o.between_names.push_back(parts[0].substr(pos, comma - pos));
                    pos = comma + 1u;
                }
                try {
                    size_t used = 0;
                    if (parts.size() > 2u) {
                        const unsigned long g = std::stoul(parts[2], &used);
                        if (used != parts[2].size() || g > 4096ul) throw Error(VOLYM_E_INVALID, usage);
                        o.between_max_gap = static_cast<uint32_t>(g);
                    }
                } catch (const std::logic_error&) { throw Error(VOLYM_E_INVALID, usage); }
                if (o.between_names.empty()) throw Error(VOLYM_E_INVALID, usage);
            }
            else if (a == "--labels-out") o.labels_out = next();
            else if (a == "--undo") o.undo = static_cast<uint32_t>(std::stoul(next()));
            else if (a == "--measure") {
                o.measure = true;
                if (i + 1 < argc && argv[i + 1][0] != '-' && std::string(argv[i + 1]) != "run" && std::string(argv[i + 1]) != "benchmark") {
                    const std::string v = next();
                    size_t pos = 0;
                    while (pos <= v.size()) {
                        const size_t comma = std::min(v.find(',', pos), v.size());
                        if (comma > pos) o.measure_names.push_back(v.substr(pos, comma - pos));
                        pos = comma + 1u;
                    }
                }
            }
            else if (a == "--surface") {
                o.surface = true;
                if (i + 1 < argc && argv[i + 1][0] != '-' && std::string(argv[i + 1]) != "run" && std::string(argv[i + 1]) != "benchmark") {
                    std::string v = next();
                    const size_t colon = v.rfind(':');
                    if (colon != std::string::npos) {
                        size_t used = 0;
                        unsigned long m = 0;
                        try { m = std::stoul(v.substr(colon + 1), &used); } catch (const std::exception&) { used = 0; }
                        if (used == 0 || used != v.size() - colon - 1 || m < 1 || m > 255) throw Error(VOLYM_E_INVALID, "--surface: NAME[,NAME...][:MIN_BYTE], MIN_BYTE in 1..255");
                        o.surface_min_byte = static_cast<uint32_t>(m);
                        v = v.substr(0, colon);
                    }
                    size_t pos = 0;
                    while (pos <= v.size()) {
                        const size_t comma = std::min(v.find(',', pos), v.size());
                        if (comma > pos) o.surface_names.push_back(v.substr(pos, comma - pos));
                        pos = comma + 1u;
                    }
                }
            }
            else if (a == "--components") {
                o.components = true;
                if (i + 1 < argc && argv[i + 1][0] != '-' && std::string(argv[i + 1]) != "run" && std::string(argv[i + 1]) != "benchmark") {
                    std::string v = next();
                    const size_t colon = v.rfind(':');
                    if (colon != std::string::npos) {
                        size_t used = 0;
                        unsigned long m = 0;
                        try { m = std::stoul(v.substr(colon + 1), &used); } catch (const std::exception&) { used = 0; }
                        if (used == 0 || used != v.size() - colon - 1 || m < 1 || m > 255) throw Error(VOLYM_E_INVALID, "--components: NAME[,NAME...][:MIN_BYTE], MIN_BYTE in 1..255");
                        o.components_min_byte = static_cast<uint32_t>(m);
                        v = v.substr(0, colon);
                    }
                    size_t pos = 0;
                    while (pos <= v.size()) {
                        const size_t comma = std::min(v.find(',', pos), v.size());
                        if (comma > pos) o.components_names.push_back(v.substr(pos, comma - pos));
                        pos = comma + 1u;
                    }
                }
            }
            else if (a == "--distance-inside") o.distance_inside = true;
            else if (a == "--distance") {
                o.distance = true;
                if (i + 1 < argc && argv[i + 1][0] != '-' && std::string(argv[i + 1]) != "run" && std::string(argv[i + 1]) != "benchmark") {
                    std::string v = next();
                    const size_t colon = v.rfind(':');
                    if (colon != std::string::npos) {
                        size_t used = 0;
                        unsigned long m = 0;
                        try { m = std::stoul(v.substr(colon + 1), &used); } catch (const std::exception&) { used = 0; }
                        if (used == 0 || used != v.size() - colon - 1 || m < 1 || m > 255) throw Error(VOLYM_E_INVALID, "--distance: NAME[,NAME...][:MIN_BYTE], MIN_BYTE in 1..255");
                        o.distance_min_byte = static_cast<uint32_t>(m);
                        v = v.substr(0, colon);
                    }
                    size_t pos = 0;
                    while (pos <= v.size()) {
                        const size_t comma = std::min(v.find(',', pos), v.size());
                        if (comma > pos) o.distance_names.push_back(v.substr(pos, comma - pos));
                        pos = comma + 1u;
                    }
                }
            }
            else if (a == "--surface-out") {
                o.surface_out = next();
                const size_t n = o.surface_out.size();
                std::string ext = n >= 4 ? o.surface_out.substr(n - 4) : std::string();
                for (char& ch : ext) ch = static_cast<char>(std::tolower(static_cast<unsigned char>(ch)));
                if (ext != ".stl") throw Error(VOLYM_E_INVALID, "--surface-out: a file ending in .stl (the Python CLI also writes .obj)");
            }
            else if (a == "--project") {
                const std::string v = next();
                const size_t comma = v.find(',');
                std::string mode = v.substr(0, comma);
                for (char& ch : mode) ch = static_cast<char>(std::toupper(static_cast<unsigned char>(ch)));
                size_t used = 0;
                float step = 0.0f;
                if (comma != std::string::npos) { try { step = std::stof(v.substr(comma + 1), &used); } catch (const std::exception&) { used = 0; } }
                if ((mode != "MAX" && mode != "MEAN") || (comma != std::string::npos && (used == 0 || used != v.size() - comma - 1 || !(step > 0.0f))))
                    throw Error(VOLYM_E_INVALID, "--project: MAX or MEAN, then optionally the distance between samples");
                o.project_mode = mode == "MEAN" ? VOLYM_PROJECT_MEAN : VOLYM_PROJECT_MAX;
                o.project_step = step;
            }
            else { std::fprintf(stderr, "usage: volym [run simple | benchmark] [-d] [--volume f --labels f --segments f] [--width n --height n] [--secs s] [--output f] [--frames-in-flight 1|2] [--crop x0,y0,z0,x1,y1,z1] [--clip-plane nx,ny,nz,px,py,pz] [--hide l,l,...] [--slice x|y|z,index] [--project MAX|MEAN[,step]] [--measure [name,...]] [--surface [name,...][:min_byte]] [--surface-out file.stl] [--components [name,...][:min_byte]] [--distance [name,...][:min_byte]] [--distance-inside] [--relabel from[,from...]:to] [--brush x,y,z[/x,y,z...]:to:r2] [--lasso x,y/x,y/x,y[/...]:from[,from...]:to] [--smooth [name,...][:r[,r,r]]] [--undo n] [--labels-out file]\n"); return 2; }
        } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 2; }
    }
    try {
        return o.command == "benchmark" ? benchmark_all(o) : run_simple(o);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
