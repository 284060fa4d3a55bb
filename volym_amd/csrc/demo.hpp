// C++ face of the compute-plugin boundary, over the C ABI of libvolym_hip.so.
//
//     trait ComputeDemo { init(ctx, state, output); update_gpu_state(ctx, state); compute_pass(ctx) }
//                                                         -- /root/reference/src/demos/mod.rs:9-17
//     struct Simple                                       -- /root/reference/src/demos/simple/mod.rs:26-121
//
// GpuContext stands where src/gpu_context.rs + GpuWriteTexture2D stood: a device and a W x H rgba8 output.
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/volym_host.h"
#include "scene.hpp"

namespace volym {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error("volym error " + std::to_string(c) + ": " + m), code(c) {}
};

class GpuContext {
public:
    GpuContext(uint32_t width, uint32_t height, int device_id = -1) : width(width), height(height)
    {
        const int rc = volym_create(&ctx_, width, height, device_id);
        if (rc != VOLYM_OK) throw Error(rc, volym_last_error(nullptr));
    }
    ~GpuContext() { volym_destroy(ctx_); }
    GpuContext(const GpuContext&) = delete;
    GpuContext& operator=(const GpuContext&) = delete;
    volym_ctx* handle() const { return ctx_; }
    void check(int rc) const { if (rc != VOLYM_OK) throw Error(rc, volym_last_error(ctx_)); }
    const uint32_t width, height;

private:
    volym_ctx* ctx_ = nullptr;
};

class ComputeDemo {
public:
    virtual ~ComputeDemo() = default;
    virtual void update_gpu_state(const GpuContext& ctx, const volym_state& state) = 0;
    virtual void compute_pass(const GpuContext& ctx) = 0;
};

// The assets Simple::init reads from hard-coded paths (src/demos/simple/mod.rs:40-55), passed explicitly.
struct SimpleAssets {
    std::vector<uint8_t> volume_raw, labels_raw;
    std::vector<SegmentInfo> segments;
    uint32_t nx = 256, ny = 256, nz = 256;       // src/gpu_resources/volume.rs:41
    int filter = VOLYM_FILTER_NEAREST;           // src/gpu_resources/volume.rs:92-95
};

// How Simple::highlight draws: colours, ring width, the alpha_min of the pick pass behind it, and where the image goes.
struct Highlight {
    uint8_t ring_rgba[4] = {255, 255, 0, 255};
    uint8_t fill_rgba[4] = {255, 255, 0, 48};
    uint32_t radius = 2;                     // 1..8
    float alpha_min = 0.5f;
    void* target_rgba8 = nullptr;            // device memory of W * H * 4 bytes; NULL: the context's own target (volym_read_outline)
};

// How Simple::slice draws: what the plane shows, the overlays, their colours, and where the image goes.
struct SliceView {
    uint32_t mode = VOLYM_SLICE_DENSITY;     // VOLYM_SLICE_DENSITY, VOLYM_SLICE_TF or VOLYM_SLICE_IMPORTANCE
    bool labels = true;                      // the segments as a colour overlay (needs label bytes in the assets)
    bool mark_cut = true;                    // tint the texels the crop box, the clip plane and the hidden segments remove
    bool uncut = false;                      // show the density before the cuts
    uint8_t strength = 96;                   // alpha of the overlay's colours
    uint8_t cut_rgba[4] = {255, 0, 0, 96};
    uint8_t background[4] = {0, 0, 0, 255};
    void* target_rgba8 = nullptr;            // device memory of width * height * 4 bytes; NULL: the context's own target (volym_read_slice)
};

// How Simple::project draws: what the image shows, the overlays, and the rect.  Records and image go to the context's own buffers.
struct ProjectView {
    float step = 0.0f;                       // distance between samples; 0: the march's dense step, 0.25 * raymarching_step_size
    bool tf = false;                         // colour through the transfer function
    bool labels = true;                      // MAX: the segment of the brightest sample as a colour overlay
    bool no_skip = false;                    // read every sample (the A/B partner of the default path)
    uint8_t strength = 96;                   // alpha of the overlay's colours
    uint8_t background[4] = {0, 0, 0, 255};
    const uint32_t* rect = nullptr;          // {x0, y0, w, h}; NULL: the whole frame
};

class Simple : public ComputeDemo {
public:
    static Simple init(const GpuContext& ctx, const volym_state& state, const SimpleAssets& a)
    {
        const size_t n = static_cast<size_t>(a.nx) * a.ny * a.nz;
        std::vector<uint8_t> vol(n), imp(n), labels(a.labels_raw);
        prepare_volume(a.volume_raw.data(), a.volume_raw.size(), a.nx, a.ny, a.nz, true, vol.data());   // GpuVolume::init
        std::vector<uint8_t> lv, im;
        for (const SegmentInfo& s : a.segments) { lv.push_back(s.label_value); im.push_back(s.importance); }
        map_segments_to_importance(labels.data(), labels.size(), lv.data(), im.data(), lv.size());       // GpuImportances::init
        prepare_volume(labels.data(), labels.size(), a.nx, a.ny, a.nz, true, imp.data());
        ctx.check(volym_set_volume(ctx.handle(), vol.data(), a.nx, a.ny, a.nz, a.filter));
        ctx.check(volym_set_importances(ctx.handle(), imp.data(), a.nx, a.ny, a.nz));
        const std::vector<uint8_t> lut = TransferFunction::default_().bake_rgba8();                       // src/demos/simple/mod.rs:64-66
        ctx.check(volym_set_transfer_function(ctx.handle(), lut.data(), 256));
        Simple s;
        s.update_gpu_state(ctx, state);
        return s;
    }
    void update_gpu_state(const GpuContext& ctx, const volym_state& state) override   // src/demos/pipeline.rs:208-212
    {
        volym_camera_uniforms cam;
        volym_parameter_uniforms par;
        if (!camera_uniforms_from(state.camera, cam)) throw Error(VOLYM_E_INVALID, "inverse_view_proj inversion failed");
        parameter_uniforms_from(state, par);
        ctx.check(volym_update(ctx.handle(), &cam, &par));
        camera_ = cam;                 // (lasso: the view of the latest frame)
        records_current_ = false;      // (highlight: the pick records of the old view are stale)
        for (int i = 0; i < 3; ++i) eye_[i] = state.camera.position[i];      // (clip_at: the plane faces the eye)
        dense_step_ = 0.25f * par.raymarching_step_size;                     // (project: the march's dense step)
    }
    void compute_pass(const GpuContext& ctx) override { ctx.check(volym_compute_pass(ctx.handle())); }   // src/demos/pipeline.rs:62-102

    // New: the label map stays on the device, and set_segments changes segment importances without a host map or an upload.
    void set_labels(const GpuContext& ctx, const SimpleAssets& a)
    {
        std::vector<uint8_t> labels(static_cast<size_t>(a.nx) * a.ny * a.nz);
        prepare_volume(a.labels_raw.data(), a.labels_raw.size(), a.nx, a.ny, a.nz, true, labels.data());
        ctx.check(volym_set_labels(ctx.handle(), labels.data(), a.nx, a.ny, a.nz));
        labels_on_device_ = true;
        records_current_ = false;
    }
    // The reference maps labels before padding them (importance.rs:148-158), so padding has importance 0 there and table[0]
    // here: with padding and table[0] != 0 this falls back to the host map (which drops the labels from the device).
    void set_segments(const GpuContext& ctx, const SimpleAssets& a, const std::vector<SegmentInfo>& segments)
    {
        const std::vector<uint8_t> table = segment_table(segments);
        const size_t n = static_cast<size_t>(a.nx) * a.ny * a.nz;
        records_current_ = false;
        if (a.labels_raw.size() < n && table[0] != 0) {
            std::vector<uint8_t> mapped(a.labels_raw), imp(n);
            std::vector<uint8_t> lv, im;
            for (const SegmentInfo& s : segments) { lv.push_back(s.label_value); im.push_back(s.importance); }
            map_segments_to_importance(mapped.data(), mapped.size(), lv.data(), im.data(), lv.size());
            prepare_volume(mapped.data(), mapped.size(), a.nx, a.ny, a.nz, true, imp.data());
            ctx.check(volym_set_importances(ctx.handle(), imp.data(), a.nx, a.ny, a.nz));
            labels_on_device_ = false;
            return;
        }
        if (!labels_on_device_) set_labels(ctx, a);
        ctx.check(volym_set_segment_importances(ctx.handle(), table.data()));
    }
    // New: relabel segments on the device by the table alone (volym_edit_labels): every texel of a segment in `from` (names, ids or
    // label values as text) gets the label of `to`, which must name a segment of the table or be a label value.  The importances are
    // mapped from the labels through the segments' table first, so that they follow the edit.
    volym_relabel_result relabel(const GpuContext& ctx, const SimpleAssets& a, const std::vector<std::string>& from, const std::string& to)
    {
        set_segments(ctx, a, a.segments);
        if (!labels_on_device_) throw Error(VOLYM_E_STATE, "relabel: the labels are shorter than the volume and label 0 is important: they cannot stay on the device");
        volym_relabel r{};
        r.box[3] = a.nx; r.box[4] = a.ny; r.box[5] = a.nz;
        r.max_byte = 255u;
        for (int l = 0; l < 256; ++l) r.to[l] = static_cast<uint8_t>(l);
        const uint8_t target = label_value_of(a, to);
        for (const std::string& s : from) r.to[label_value_of(a, s)] = target;
        volym_relabel_result out{};
        ctx.check(volym_edit_labels(ctx.handle(), &r, &out));
        records_current_ = false;
        return out;
    }
    // New: one stroke of the brush on the device (volym_brush_labels): the texels within sqrt(r2) texels of the polyline of `points`
    // (texels of the prepared volume, as a pick reports them; at most VOLYM_BRUSH_MAX_POINTS), whatever their label, get the label of
    // `to`, which must name a segment of the table or be a label value.  One call, one step of the history.
    volym_relabel_result brush(const GpuContext& ctx, const SimpleAssets& a, const std::vector<std::array<uint32_t, 3>>& points, const std::string& to, uint32_t r2)
    {
        set_segments(ctx, a, a.segments);
        if (!labels_on_device_) throw Error(VOLYM_E_STATE, "brush: the labels are shorter than the volume and label 0 is important: they cannot stay on the device");
        if (points.empty() || points.size() > VOLYM_BRUSH_MAX_POINTS) throw Error(VOLYM_E_INVALID, "brush: 1..256 points");
        volym_brush b{};
        b.box[3] = a.nx; b.box[4] = a.ny; b.box[5] = a.nz;
        b.max_byte = 255u;
        const uint8_t target = label_value_of(a, to);
        for (int l = 0; l < 256; ++l) b.to[l] = target;
        b.weight[0] = b.weight[1] = b.weight[2] = 1u;
        b.r2 = r2;
        b.n_points = static_cast<uint32_t>(points.size());
        for (size_t i = 0; i < points.size(); ++i) {
            for (int k = 0; k < 3; ++k) if (points[i][k] > 0xffffu) throw Error(VOLYM_E_INVALID, "brush: a point lies outside the volume");
            b.points[i].x = static_cast<uint16_t>(points[i][0]); b.points[i].y = static_cast<uint16_t>(points[i][1]); b.points[i].z = static_cast<uint16_t>(points[i][2]);
        }
        volym_relabel_result out{};
        ctx.check(volym_brush_labels(ctx.handle(), &b, &out));
        records_current_ = false;
        return out;
    }
    // New: scissors on the device (volym_lasso_labels): the texels of the segments `from` (names, ids or label values as text) that the
    // latest frame's view projects into the polygon `pixels` (3 to VOLYM_LASSO_MAX_POINTS vertices, closed implicitly, even-odd; they
    // may lie off screen), through the whole volume, get the label of `to`.  One call, one step of the history.
    volym_relabel_result lasso(const GpuContext& ctx, const SimpleAssets& a, const std::vector<std::array<int32_t, 2>>& pixels, const std::vector<std::string>& from,
                               const std::string& to)
    {
        set_segments(ctx, a, a.segments);
        if (!labels_on_device_) throw Error(VOLYM_E_STATE, "lasso: the labels are shorter than the volume and label 0 is important: they cannot stay on the device");
        if (pixels.size() < 3u || pixels.size() > VOLYM_LASSO_MAX_POINTS) throw Error(VOLYM_E_INVALID, "lasso: 3..1024 vertices");
        std::vector<volym_lasso> request(1);                                 // (8576 bytes: off the stack)
        volym_lasso& l = request[0];
        l.box[3] = a.nx; l.box[4] = a.ny; l.box[5] = a.nz;
        l.max_byte = 255u;
        for (int k = 0; k < 256; ++k) l.to[k] = static_cast<uint8_t>(k);
        const uint8_t target = label_value_of(a, to);
        for (const std::string& s : from) l.to[label_value_of(a, s)] = target;
        const uint32_t dims[3] = {a.nx, a.ny, a.nz};
        ctx.check(volym_lasso_view_from_camera(&camera_, ctx.width, ctx.height, dims, 0.0, &l.view));
        l.n_points = static_cast<uint32_t>(pixels.size());
        for (size_t i = 0; i < pixels.size(); ++i) { l.points[i].x = pixels[i][0]; l.points[i].y = pixels[i][1]; }
        volym_relabel_result out{};
        ctx.check(volym_lasso_labels(ctx.handle(), &l, &out));
        records_current_ = false;
        return out;
    }
    // New: smoothing on the device (volym_smooth_labels): one pass of the majority filter over `radius` texels per axis, through the
    // whole volume.  names empty: joint, every label gives and takes; else those segments (names, ids or label values as text) and
    // label 0 give and take.  One call, one step of the history.
    volym_relabel_result smooth(const GpuContext& ctx, const SimpleAssets& a, const std::vector<std::string>& names, const std::array<uint32_t, 3>& radius)
    {
        set_segments(ctx, a, a.segments);
        if (!labels_on_device_) throw Error(VOLYM_E_STATE, "smooth: the labels are shorter than the volume and label 0 is important: they cannot stay on the device");
        volym_smooth s{};
        s.box[3] = a.nx; s.box[4] = a.ny; s.box[5] = a.nz;
        s.max_byte = 255u;
        for (int k = 0; k < 3; ++k) s.radius[k] = radius[static_cast<size_t>(k)];
        for (int k = 0; k < 256; ++k) s.give[k] = s.take[k] = names.empty() ? 1u : 0u;
        if (!names.empty()) s.give[0] = s.take[0] = 1u;
        for (const std::string& n : names) { const uint8_t l = label_value_of(a, n); s.give[l] = s.take[l] = 1u; }
        volym_relabel_result out{};
        ctx.check(volym_smooth_labels(ctx.handle(), &s, &out));
        records_current_ = false;
        return out;
    }
    // New: grow several segments at once (volym_nearest_pass, volym_fill_labels): one nearest pass from the union of `names` (names,
    // ids or label values as text; empty: every label but 0), then one fill -- every unlabelled texel with a density byte above 0
    // joins the segment it is nearest to, the first in (z, y, x) among equals, if that is at most r texels away (r < 0: however far).
    // One call, one step of the history.
    volym_relabel_result fill(const GpuContext& ctx, const SimpleAssets& a, const std::vector<std::string>& names, double r)
    {
        set_segments(ctx, a, a.segments);
        if (!labels_on_device_) throw Error(VOLYM_E_STATE, "fill: the labels are shorter than the volume and label 0 is important: they cannot stay on the device");
        volym_distance d{};
        d.box[3] = a.nx; d.box[4] = a.ny; d.box[5] = a.nz;
        d.min_byte = 1u;
        d.weight[0] = d.weight[1] = d.weight[2] = 1u;
        if (names.empty()) std::memset(d.select + 1, 1, 255);
        for (const std::string& n : names) d.select[label_value_of(a, n)] = 1u;
        d.select[0] = 0u;
        ctx.check(volym_nearest_pass(ctx.handle(), &d));
        volym_fill f{};
        std::memcpy(f.box, d.box, sizeof f.box);
        f.min_byte = 1u; f.max_byte = 255u;
        f.give[0] = 1u;
        std::memcpy(f.take, d.select, 256);
        f.d2_hi = r < 0.0 ? 0xffffffffu : static_cast<uint32_t>(std::floor(r * r + 1e-9));
        volym_relabel_result out{};
        ctx.check(volym_fill_labels(ctx.handle(), &f, &out));
        records_current_ = false;
        return out;
    }
    // New: grow several segments at once through the matter alone (volym_geodesic_pass, volym_flood_labels): one geodesic pass from
    // the union of `names` (names, ids or label values as text; empty: every label but 0) through the unlabelled texels with a
    // density byte above 0, at most r steps (r < 0: however far), then one flood -- every texel reached joins the segment whose seed
    // is the fewest 6-connected steps away, the smallest label among equals.  A gap of air is no bridge.  One step of the history.
    volym_relabel_result flood(const GpuContext& ctx, const SimpleAssets& a, const std::vector<std::string>& names, double r)
    {
        set_segments(ctx, a, a.segments);
        if (!labels_on_device_) throw Error(VOLYM_E_STATE, "flood: the labels are shorter than the volume and label 0 is important: they cannot stay on the device");
        if (r >= 0.0 && (r < 1.0 || r > static_cast<double>(VOLYM_GEODESIC_STEPS_MAX))) throw Error(VOLYM_E_INVALID, "flood: R is a number of steps, 1 at least");
        auto g = std::make_unique<volym_geodesic>();       // (1324 bytes, zeroed)
        g->box[3] = a.nx; g->box[4] = a.ny; g->box[5] = a.nz;
        g->min_byte = 1u; g->max_byte = 255u;
        if (names.empty()) std::memset(g->seed + 1, 1, 255);
        for (const std::string& n : names) g->seed[label_value_of(a, n)] = 1u;
        g->seed[0] = 0u;
        g->through[0] = 1u;
        g->max_steps = r < 0.0 ? 0u : static_cast<uint32_t>(r);
        ctx.check(volym_geodesic_pass(ctx.handle(), g.get()));
        volym_flood f{};
        std::memcpy(f.box, g->box, sizeof f.box);
        f.max_byte = 255u;
        f.give[0] = 1u;
        std::memcpy(f.take, g->seed, 256);
        for (int l = 0; l < 256; ++l) f.to[l] = static_cast<uint8_t>(l);
        f.steps_lo = 1u; f.steps_hi = 0xffffffffu;
        volym_relabel_result out{};
        ctx.check(volym_flood_labels(ctx.handle(), &f, &out));
        records_current_ = false;
        return out;
    }
    // New: grow from seeds (volym_cost_pass, volym_spread_labels): one cost pass from the union of `names` (names, ids or label values
    // as text; at least one) through the unlabelled texels with a density byte above 0, where a step costs 1 and `contrast` per byte of
    // density change across it, at most max_cost in all (0: however much), then one spread -- every texel reached joins the segment
    // that reaches it most cheaply, the smallest label among equals.  One step of the history.
    volym_relabel_result grow_from_seeds(const GpuContext& ctx, const SimpleAssets& a, const std::vector<std::string>& names, uint32_t contrast, uint32_t max_cost)
    {
        set_segments(ctx, a, a.segments);
        if (!labels_on_device_) throw Error(VOLYM_E_STATE, "grow from seeds: the labels are shorter than the volume and label 0 is important: they cannot stay on the device");
        if (names.empty()) throw Error(VOLYM_E_INVALID, "grow from seeds: name the segments that grow");
        auto q = std::make_unique<volym_cost>();           // (1336 bytes, zeroed)
        q->box[3] = a.nx; q->box[4] = a.ny; q->box[5] = a.nz;
        q->min_byte = 1u; q->max_byte = 255u;
        for (const std::string& n : names) q->seed[label_value_of(a, n)] = 1u;
        q->seed[0] = 0u;
        q->through[0] = 1u;
        q->step_cost = 1u; q->contrast_cost = contrast; q->max_cost = max_cost; q->hist_shift = 8u;
        ctx.check(volym_cost_pass(ctx.handle(), q.get()));
        volym_spread s{};
        std::memcpy(s.box, q->box, sizeof s.box);
        s.max_byte = 255u;
        s.give[0] = 1u;
        std::memcpy(s.take, q->seed, 256);
        for (int l = 0; l < 256; ++l) s.to[l] = static_cast<uint8_t>(l);
        s.cost_lo = 1u; s.cost_hi = 0xffffffffu;
        volym_relabel_result out{};
        ctx.check(volym_spread_labels(ctx.handle(), &s, &out));
        records_current_ = false;
        return out;
    }
    // New: fill between slices (volym_interpolate_pass, volym_interpolate_labels): each segment of `names` (names, ids or label values
    // as text; at least one), painted on some slices perpendicular to `axis` (0, 1, 2), is interpolated across the slices between them
    // -- one pass and one edit per segment, each one step of the history.  The unlabelled texels the interpolated shape holds join the
    // segment; gaps of more than max_gap slices are left alone (0: no limit).  Returns per segment its label, the summary's counts and the
    // edit's result.
    struct FilledBetween { uint32_t label, n_keys, n_gaps, n_gap_slices, n_refused; volym_relabel_result result; };
    std::vector<FilledBetween> fill_between(const GpuContext& ctx, const SimpleAssets& a, const std::vector<std::string>& names, uint32_t axis, uint32_t max_gap)
    {
        set_segments(ctx, a, a.segments);
        if (!labels_on_device_) throw Error(VOLYM_E_STATE, "fill between: the labels are shorter than the volume and label 0 is important: they cannot stay on the device");
        if (names.empty()) throw Error(VOLYM_E_INVALID, "fill between: name the segments to interpolate");
        std::vector<FilledBetween> out;
        auto summary = std::make_unique<volym_interpolate_summary>();      // (65592 bytes)
        for (const std::string& n : names) {
            const uint32_t l = label_value_of(a, n);
            volym_interpolate q{};
            q.box[3] = a.nx; q.box[4] = a.ny; q.box[5] = a.nz;
            q.select[l] = 1u;
            q.weight[0] = q.weight[1] = q.weight[2] = 1u;
            q.axis = axis; q.max_gap = max_gap;
            ctx.check(volym_interpolate_pass(ctx.handle(), &q));
            volym_interpolate_edit e{};
            std::memcpy(e.box, q.box, sizeof e.box);
            e.max_byte = 255u;
            for (int k = 0; k < 256; ++k) e.to[k] = e.out[k] = static_cast<uint8_t>(k);
            e.to[0] = static_cast<uint8_t>(l);
            FilledBetween f{};
            ctx.check(volym_interpolate_labels(ctx.handle(), &e, &f.result));
            ctx.check(volym_read_interpolate(ctx.handle(), summary.get()));
            f.label = l; f.n_keys = summary->n_keys; f.n_gaps = summary->n_gaps; f.n_gap_slices = summary->n_gap_slices; f.n_refused = summary->n_refused;
            out.push_back(f);
        }
        records_current_ = false;
        return out;
    }
    // New: keep a history of the label edits in at most budget_bytes of device memory (volym_label_history), so that undo can take
    // them back.  The labels go to the device first: handing them to the context clears the history.
    void history(const GpuContext& ctx, const SimpleAssets& a, uint64_t budget_bytes = 256ull << 20)
    {
        set_segments(ctx, a, a.segments);
        if (!labels_on_device_) throw Error(VOLYM_E_STATE, "history: the labels are shorter than the volume and label 0 is important: they cannot stay on the device");
        ctx.check(volym_label_history(ctx.handle(), budget_bytes));
    }
    // New: take the latest edit back on the device (volym_undo_labels).  False: there is nothing to take back.
    bool undo(const GpuContext& ctx, volym_relabel_result& out)
    {
        struct volym_label_history_info info{};
        ctx.check(volym_label_history_info(ctx.handle(), &info));
        if (info.undo_steps == 0u) return false;
        ctx.check(volym_undo_labels(ctx.handle(), &out));
        records_current_ = false;
        return true;
    }
    // New: the labels as they stand on the device, as raw bytes in the orientation prepare_volume read (the y flip undone)
    std::vector<uint8_t> labels_from_device(const GpuContext& ctx, const SimpleAssets& a)
    {
        if (!labels_on_device_) set_labels(ctx, a);
        std::vector<uint8_t> prepared(static_cast<size_t>(a.nx) * a.ny * a.nz), raw(prepared.size());
        ctx.check(volym_read_labels(ctx.handle(), nullptr, prepared.data()));
        const size_t row = a.nx;
        for (size_t z = 0; z < a.nz; ++z)
            for (size_t y = 0; y < a.ny; ++y)
                std::copy(prepared.begin() + (z * a.ny + y) * row, prepared.begin() + (z * a.ny + y + 1) * row, raw.begin() + (z * a.ny + (a.ny - 1 - y)) * row);
        return raw;
    }
    // New: axis-aligned crop box in unit-cube coordinates in [0, 1] (the cube the camera orbits; y as the prepared, flipped volume
    // has it): texel = floor(p * n + 0.5) clamped to [0, n].  Density and importances outside it count as 0 (volym_set_crop_box).
    void set_crop(const GpuContext& ctx, const SimpleAssets& a, const float lo01[3], const float hi01[3])
    {
        const uint32_t n[3] = {a.nx, a.ny, a.nz};
        uint32_t lo[3], hi[3];
        for (int i = 0; i < 3; ++i) { lo[i] = crop_texel(lo01[i], n[i]); hi[i] = crop_texel(hi01[i], n[i]); }
        ctx.check(volym_set_crop_box(ctx.handle(), lo, hi));
        records_current_ = false;
    }
    // New: oblique clip plane through `point` with the given normal, both in the unit-cube coordinates set_crop takes: what lies on
    // the side the normal points to is cut away (volym_set_clip_plane).  The integers, in double: g_i = normal_i / n_i,
    // k = 4096 / max|g_i|, a_i = floor(g_i * k + 0.5), d = floor(sum a_i * (point_i * n_i - 0.5)).  normal == NULL lifts the plane.
    struct ClipPlane { int32_t n[3]; int32_t d; };
    ClipPlane set_clip_plane(const GpuContext& ctx, const SimpleAssets& a, const float normal[3], const float point[3])
    {
        ClipPlane p{{0, 0, 0}, 0};
        if (normal) p = clip_plane_texels(a, normal, point);
        ctx.check(volym_set_clip_plane(ctx.handle(), p.n, p.d));
        records_current_ = false;
        return p;
    }
    static ClipPlane clip_plane_texels(const SimpleAssets& a, const float normal[3], const float point[3])
    {
        const double dims[3] = {static_cast<double>(a.nx), static_cast<double>(a.ny), static_cast<double>(a.nz)};
        double g[3], top = 0.0, sum = 0.0;
        for (int i = 0; i < 3; ++i) { g[i] = static_cast<double>(normal[i]) / dims[i]; top = std::max(top, std::fabs(g[i])); }
        if (!(top > 0.0) || !std::isfinite(top)) throw Error(VOLYM_E_INVALID, "clip plane: the normal must be finite and not zero");
        ClipPlane p{};
        for (int i = 0; i < 3; ++i) {
            const double c = std::floor(g[i] * (4096.0 / top) + 0.5);
            p.n[i] = static_cast<int32_t>(c);
            sum += c * (static_cast<double>(point[i]) * dims[i] - 0.5);
        }
        sum = std::floor(sum);
        if (!(sum >= -2147483648.0 && sum <= 2147483647.0)) throw Error(VOLYM_E_INVALID, "clip plane: the point is too far from the volume");
        p.d = static_cast<int32_t>(sum);
        return p;
    }
    // New: hide the segments with the given label values and show all others (volym_set_segment_visibility).  The labels go to the
    // device first if they are not there yet; the importances stay what they were.
    void set_hidden(const GpuContext& ctx, const SimpleAssets& a, const std::vector<uint8_t>& hidden_label_values)
    {
        uint8_t visible[256];
        for (int l = 0; l < 256; ++l) visible[l] = 1;
        for (uint8_t l : hidden_label_values) visible[l] = 0;
        if (!labels_on_device_) {
            if (hidden_label_values.empty()) return;
            set_labels(ctx, a);
        }
        ctx.check(volym_set_segment_visibility(ctx.handle(), visible));
        records_current_ = false;
    }
    // New: what pixel (x, y) of the frame shows -- the first sample of its ray after which alpha >= alpha_min (volym_pick): the
    // record, the name of the segment with its label (empty: none, or no labels) and the texel's centre in the unit-cube
    // coordinates set_crop takes.  The labels go to the device first if they are not there yet.
    struct Picked {
        volym_pick_record record;
        std::string segment;
        float pos[3];
    };
    Picked pick(const GpuContext& ctx, const SimpleAssets& a, uint32_t x, uint32_t y, float alpha_min = 0.5f)
    {
        if (!labels_on_device_ && !a.labels_raw.empty()) set_labels(ctx, a);
        Picked p{};
        ctx.check(volym_pick(ctx.handle(), x, y, alpha_min, &p.record));
        records_current_ = false;      // (the one-pixel pass took the place of a whole frame's records)
        describe(a, p);
        return p;
    }
    // New: outline and tint segments in the frame of the latest compute pass (volym_outline_pass) -- one outline pass over the
    // records of a whole-frame pick pass, which runs only if the demo has none for the current view and scene (update_gpu_state,
    // set_crop, set_clip_plane, set_hidden, set_segments and set_labels make the records stale).  `segments`: names or ids of the segments table, or
    // label values written as numbers ("3").  The image goes to target_rgba8 (device memory), or with NULL to the context's own
    // target (volym_read_outline).  Returns the selected label values.
    std::vector<uint8_t> highlight(const GpuContext& ctx, const SimpleAssets& a, const std::vector<std::string>& segments, const Highlight& h = Highlight())
    {
        std::vector<uint8_t> values;
        for (const std::string& s : segments) values.push_back(label_value_of(a, s));
        highlight_labels(ctx, a, values, h);
        return values;
    }
    // New: hover -- outline the segment pixel (x, y) shows (nothing when it shows no labelled sample: the image is then the frame).
    // The label comes from the current records, which are read back once per view and scene: the hovers after the first cost the
    // outline pass alone.  Returns what pick returns.
    Picked highlight_at(const GpuContext& ctx, const SimpleAssets& a, uint32_t x, uint32_t y, const Highlight& h = Highlight())
    {
        if (x >= ctx.width || y >= ctx.height) throw Error(VOLYM_E_INVALID, "highlight_at: the pixel is not inside the frame");
        current_records(ctx, a, h.alpha_min);
        if (records_host_.empty()) {
            records_host_.resize(static_cast<size_t>(ctx.width) * ctx.height);
            ctx.check(volym_read_picks(ctx.handle(), records_host_.data()));
        }
        Picked p{};
        p.record = records_host_[static_cast<size_t>(y) * ctx.width + x];
        describe(a, p);
        std::vector<uint8_t> values;
        if (p.record.status == 2 && p.record.has_labels) values.push_back(p.record.label);
        highlight_labels(ctx, a, values, h);
        return p;
    }

private:
    // a whole-frame pick pass, unless the records of one for the current view, scene and alpha_min are there already
    void current_records(const GpuContext& ctx, const SimpleAssets& a, float alpha_min)
    {
        if (!labels_on_device_ && !a.labels_raw.empty()) set_labels(ctx, a);
        if (records_current_ && records_alpha_min_ == alpha_min) return;
        ctx.check(volym_pick_pass(ctx.handle(), nullptr, alpha_min));
        records_current_ = true;
        records_alpha_min_ = alpha_min;
        records_host_.clear();
    }
    void highlight_labels(const GpuContext& ctx, const SimpleAssets& a, const std::vector<uint8_t>& values, const Highlight& h)
    {
        current_records(ctx, a, h.alpha_min);
        volym_outline o{};
        for (uint8_t l : values) o.selected[l] = 1;
        for (int i = 0; i < 4; ++i) { o.ring_rgba[i] = h.ring_rgba[i]; o.fill_rgba[i] = h.fill_rgba[i]; }
        o.radius = h.radius;
        ctx.check(volym_outline_pass(ctx.handle(), &o, nullptr, nullptr, h.target_rgba8));
    }
    static uint8_t label_value_of(const SimpleAssets& a, const std::string& s)
    {
        for (const SegmentInfo& seg : a.segments)
            if (seg.name == s || seg.id == s) return seg.label_value;
        size_t used = 0;
        int l = -1;
        try { l = std::stoi(s, &used); } catch (...) { used = 0; }
        if (s.empty() || used != s.size() || l < 0 || l > 255) throw Error(VOLYM_E_INVALID, "no segment with name or id '" + s + "'");
        return static_cast<uint8_t>(l);
    }
    // segment name and unit-cube position of a record
    static void describe(const SimpleAssets& a, Picked& p)
    {
        const uint32_t n[3] = {a.nx, a.ny, a.nz}, t[3] = {p.record.x, p.record.y, p.record.z};
        for (int i = 0; i < 3; ++i) p.pos[i] = (static_cast<float>(t[i]) + 0.5f) / static_cast<float>(n[i]);
        if (p.record.status == 2 && p.record.has_labels)
            for (const SegmentInfo& s : a.segments)
                if (s.label_value == p.record.label) { p.segment = s.name; break; }
    }

public:
    // New: click to hide -- a pick, then set_hidden with that label added to the hidden ones.  Nothing changes when the pixel shows
    // no labelled sample.
    Picked hide_at(const GpuContext& ctx, const SimpleAssets& a, uint32_t x, uint32_t y, float alpha_min = 0.5f)
    {
        const Picked p = pick(ctx, a, x, y, alpha_min);
        if (p.record.status != 2 || !p.record.has_labels) return p;
        uint8_t visible[256];
        ctx.check(volym_get_segment_visibility(ctx.handle(), visible));
        std::vector<uint8_t> hidden;
        for (int l = 0; l < 256; ++l)
            if (!visible[l] || l == p.record.label) hidden.push_back(static_cast<uint8_t>(l));
        set_hidden(ctx, a, hidden);
        return p;
    }
    // New: click to cut -- a pick, then the clip plane through the picked texel's centre with the normal pointing from there to the
    // eye: everything between the eye and the clicked point is cut away, the texel itself stays.  False: the pixel shows nothing, and
    // the plane stays as it is.
    bool clip_at(const GpuContext& ctx, const SimpleAssets& a, uint32_t x, uint32_t y, ClipPlane& plane, float alpha_min = 0.5f)
    {
        const Picked p = pick(ctx, a, x, y, alpha_min);
        if (p.record.status != 2) return false;
        const float normal[3] = {eye_[0] - p.pos[0], eye_[1] - p.pos[1], eye_[2] - p.pos[2]};
        plane = clip_plane_texels(a, normal, p.pos);
        plane.d = plane.n[0] * p.record.x + plane.n[1] * p.record.y + plane.n[2] * p.record.z;      // exactly through the texel
        ctx.check(volym_set_clip_plane(ctx.handle(), plane.n, plane.d));
        records_current_ = false;
        return true;
    }
    // New: the slice view beside the 3-D picture -- the plane normal to `axis` (0 = x, 1 = y, 2 = z) through texel `index` of the
    // prepared volume, one texel per pixel (volym_slice_axis, volym_slice_pass).  One kernel; no update and no frame needed.  The
    // labels go to the device first if the overlay is wanted and they are not there yet.  Returns the slice, whose map
    // volym_slice_texel inverts a click with; the image goes to v.target_rgba8 or the context's own target (volym_read_slice).
    volym_slice slice(const GpuContext& ctx, const SimpleAssets& a, int axis, uint32_t index, const SliceView& v = SliceView())
    {
        volym_slice s{};
        const uint32_t dims[3] = {a.nx, a.ny, a.nz};
        ctx.check(volym_slice_axis(axis, index, dims, &s));
        s.mode = v.mode;
        s.flags = (v.mark_cut ? VOLYM_SLICE_MARK_CUT : 0u) | (v.uncut ? VOLYM_SLICE_UNCUT : 0u);
        if (v.labels && (labels_on_device_ || !a.labels_raw.empty())) {
            if (!labels_on_device_) set_labels(ctx, a);
            s.flags |= VOLYM_SLICE_LABELS;
        }
        for (int i = 0; i < 4; ++i) { s.cut_rgba[i] = v.cut_rgba[i]; s.background[i] = v.background[i]; }
        segment_palette(a, v.strength, s.palette);
        ctx.check(volym_slice_pass(ctx.handle(), &s, v.target_rgba8));
        return s;
    }
    // New: click to look inside -- the three orthogonal slices through the texel pixel (x, y) of the frame shows, read back as
    // width * height * 4 bytes each (images[axis], sizes in slices[axis]).  False: the pixel shows nothing.
    struct Slices {
        Picked picked;
        volym_slice slices[3];
        std::vector<uint8_t> images[3];
    };
    bool slices_at(const GpuContext& ctx, const SimpleAssets& a, uint32_t x, uint32_t y, Slices& out, const SliceView& v = SliceView(), float alpha_min = 0.5f)
    {
        out.picked = pick(ctx, a, x, y, alpha_min);
        if (out.picked.record.status != 2) return false;
        const uint32_t t[3] = {out.picked.record.x, out.picked.record.y, out.picked.record.z};
        slices_through(ctx, a, t, out, v);
        return true;
    }
    // the three orthogonal slices through texel t, read back into out.slices / out.images
    void slices_through(const GpuContext& ctx, const SimpleAssets& a, const uint32_t t[3], Slices& out, const SliceView& v)
    {
        SliceView own = v;
        own.target_rgba8 = nullptr;
        for (int axis = 0; axis < 3; ++axis) {
            out.slices[axis] = slice(ctx, a, axis, t[axis], own);
            out.images[axis].resize(static_cast<size_t>(out.slices[axis].width) * out.slices[axis].height * 4);
            ctx.check(volym_read_slice(ctx.handle(), out.images[axis].data()));
        }
    }
    // New: the projection view -- maximum (VOLYM_PROJECT_MAX) or mean (VOLYM_PROJECT_MEAN, the X-ray) intensity along the rays of the
    // current view, through the scene as it stands (volym_project_image_pass).  The labels go to the device first if they are not
    // there yet.  Records and image go to the context's own buffers (volym_read_projection, volym_read_projection_image).
    // Returns the request.
    volym_project project(const GpuContext& ctx, const SimpleAssets& a, uint32_t mode, const ProjectView& v = ProjectView())
    {
        if (!labels_on_device_ && !a.labels_raw.empty()) set_labels(ctx, a);      // (the records name the segment either way)
        volym_project p{};
        p.step = v.step > 0.0f ? v.step : dense_step_;
        p.mode = mode;
        p.flags = (v.tf ? VOLYM_PROJECT_TF : 0u) | (v.no_skip ? VOLYM_PROJECT_NO_SKIP : 0u);
        if (v.labels && mode == VOLYM_PROJECT_MAX && labels_on_device_) p.flags |= VOLYM_PROJECT_LABELS;
        for (int i = 0; i < 4; ++i) p.background[i] = v.background[i];
        segment_palette(a, v.strength, p.palette);
        ctx.check(volym_project_image_pass(ctx.handle(), &p, v.rect));
        return p;
    }
    // New: the brightest sample of the ray of pixel (x, y) (volym_project_at): the record, the name of the segment with its label
    // (empty: none, or no labels) and the texel's centre in the unit-cube coordinates set_crop takes.  step 0: the dense step.
    struct Projected {
        struct volym_projection record;
        std::string segment;
        float pos[3];
    };
    Projected project_at(const GpuContext& ctx, const SimpleAssets& a, uint32_t x, uint32_t y, float step = 0.0f)
    {
        if (!labels_on_device_ && !a.labels_raw.empty()) set_labels(ctx, a);
        Projected p{};
        ctx.check(volym_project_at(ctx.handle(), x, y, step > 0.0f ? step : dense_step_, &p.record));
        if (p.record.status == 2) {
            p.pos[0] = (p.record.x + 0.5f) / a.nx; p.pos[1] = (p.record.y + 0.5f) / a.ny; p.pos[2] = (p.record.z + 0.5f) / a.nz;
            if (labels_on_device_)
                for (const SegmentInfo& s : a.segments)
                    if (s.label_value == p.record.label) { p.segment = s.name; break; }
        }
        return p;
    }
    // New: click the bright spot -- the three orthogonal slices through the texel of the maximum along the ray of pixel (x, y), read
    // back as slices_at reads them (out.picked stays empty).  False: the ray shows nothing.
    bool brightest_slices_at(const GpuContext& ctx, const SimpleAssets& a, uint32_t x, uint32_t y, Projected& at, Slices& out, const SliceView& v = SliceView(),
                             float step = 0.0f)
    {
        at = project_at(ctx, a, x, y, step);
        if (at.record.status != 2) return false;
        const uint32_t t[3] = {at.record.x, at.record.y, at.record.z};
        slices_through(ctx, a, t, out, v);
        return true;
    }
    // New: measuring segments (volym_measure_pass) -- what a user reads off one record of a measurement, derived on the host in
    // double from the record's exact integers: mean and population deviation of the density byte, centroid (mean texel index, x
    // first), physical volume (count * the volume of a texel) and in_view, the share of the segment's texels that were counted
    // (from volym_label_counts; of the whole volume without labels).
    struct Measured {
        uint8_t label;
        std::string segment;                 // name in the segments table ("label N" for a value it does not list)
        struct volym_segment_stats stats;
        double mean, std_dev, centroid[3], volume, in_view;
    };
    static Measured segment_summary(const struct volym_segment_stats& r, const double spacing[3] = nullptr)
    {
        Measured m{};
        m.stats = r;
        if (r.count == 0u) return m;
        const long double n = static_cast<long double>(r.count), s = static_cast<long double>(r.sum);
        m.mean = static_cast<double>(s / n);
        // count * sum_sq - sum^2 in 128 bits: exact, so a constant segment has deviation 0
        const unsigned __int128 num = static_cast<unsigned __int128>(r.count) * r.sum_sq - static_cast<unsigned __int128>(r.sum) * r.sum;
        m.std_dev = static_cast<double>(std::sqrt(static_cast<long double>(num)) / n);
        m.centroid[0] = static_cast<double>(r.sum_x / n); m.centroid[1] = static_cast<double>(r.sum_y / n); m.centroid[2] = static_cast<double>(r.sum_z / n);
        m.volume = static_cast<double>(r.count) * (spacing ? spacing[0] * spacing[1] * spacing[2] : 1.0);
        return m;
    }
    // One measure pass plus the read over the scene as it stands (uncut: as it was uploaded), inside box01 = {x0, y0, z0, x1, y1, z1}
    // in the unit-cube coordinates set_crop takes (NULL: the whole volume).  `segments`: names, ids or label values written as
    // numbers; empty: every label value with a texel in view.  The labels go to the device first if they are not there yet; without
    // labels everything is label 0.
    std::vector<Measured> measure(const GpuContext& ctx, const SimpleAssets& a, const std::vector<std::string>& segments = {}, const float* box01 = nullptr,
                                  bool uncut = false, const double spacing[3] = nullptr)
    {
        if (!labels_on_device_ && !a.labels_raw.empty()) set_labels(ctx, a);
        volym_measure m{};
        const uint32_t n[3] = {a.nx, a.ny, a.nz};
        for (int i = 0; i < 3; ++i) { m.box[i] = box01 ? crop_texel(box01[i], n[i]) : 0u; m.box[3 + i] = box01 ? crop_texel(box01[3 + i], n[i]) : n[i]; }
        m.flags = uncut ? VOLYM_MEASURE_UNCUT : 0u;
        ctx.check(volym_measure_pass(ctx.handle(), &m));
        std::vector<struct volym_measurement> r(1);
        ctx.check(volym_read_measure(ctx.handle(), r.data()));
        uint64_t totals[256];
        for (int l = 0; l < 256; ++l) totals[l] = static_cast<uint64_t>(a.nx) * a.ny * a.nz;
        if (labels_on_device_) ctx.check(volym_label_counts(ctx.handle(), totals));
        std::vector<uint8_t> values;
        for (const std::string& s : segments) values.push_back(label_value_of(a, s));
        if (segments.empty())
            for (int l = 0; l < 256; ++l) if (r[0].seg[l].count != 0u) values.push_back(static_cast<uint8_t>(l));
        std::vector<Measured> out;
        for (uint8_t l : values) {
            Measured s = segment_summary(r[0].seg[l], spacing);
            s.label = l;
            s.segment = "label " + std::to_string(l);
            for (const SegmentInfo& seg : a.segments) if (seg.label_value == l) { s.segment = seg.name.empty() ? seg.id : seg.name; break; }
            s.in_view = totals[l] ? static_cast<double>(s.stats.count) / static_cast<double>(totals[l]) : 0.0;
            out.push_back(s);
        }
        return out;
    }
    // New: the density histogram of the visible scene (no segments), or of the given segments as far as they are visible: 256 counts,
    // the curve a transfer-function editor draws behind its control points.
    std::vector<uint64_t> histogram(const GpuContext& ctx, const SimpleAssets& a, const std::vector<std::string>& segments = {})
    {
        if (!labels_on_device_ && !a.labels_raw.empty()) set_labels(ctx, a);
        volym_measure m{};
        m.box[3] = a.nx; m.box[4] = a.ny; m.box[5] = a.nz;
        if (!segments.empty()) {
            for (int l = 0; l < 256; ++l) m.group[l] = VOLYM_MEASURE_NO_GROUP;
            for (const std::string& s : segments) m.group[label_value_of(a, s)] = 0;
        }
        ctx.check(volym_measure_pass(ctx.handle(), &m));
        std::vector<struct volym_measurement> r(1);
        ctx.check(volym_read_measure(ctx.handle(), r.data()));
        return std::vector<uint64_t>(r[0].hist[0], r[0].hist[0] + 256);
    }
    // New: click to measure -- a pick, then the summary of the segment the pixel shows.  False: it shows no labelled sample.
    bool measure_at(const GpuContext& ctx, const SimpleAssets& a, uint32_t x, uint32_t y, Measured& out, float alpha_min = 0.5f)
    {
        const Picked p = pick(ctx, a, x, y, alpha_min);
        if (p.record.status != 2 || !p.record.has_labels) return false;
        out = measure(ctx, a, {std::to_string(p.record.label)}).front();
        return true;
    }
    // New: segment surfaces (volym_surface_pass) -- what a user reads off the summary for one label: faces per direction and per
    // axis, area in physical units, the enclosed texel count from the divergence sums (pos - neg, equal on the three axes when the
    // label was selected alone) beside the measured count, and sphericity pi^(1/3) (6 V)^(2/3) / A with V from the measured count.
    struct Surfaced {
        uint8_t label;
        std::string segment;
        uint64_t faces[6], pairs[3], enclosed, measured;
        double area, volume, sphericity;
    };
    // One surface pass per segment -- each selected alone, so that its surface is closed and includes the faces it shares with other
    // segments -- and one measure pass, over the scene as it stands (uncut: as it was uploaded).  `segments` as measure takes them;
    // min_byte: the density byte from which a texel is solid.  Segments without faces are left out.
    std::vector<Surfaced> surface(const GpuContext& ctx, const SimpleAssets& a, const std::vector<std::string>& segments = {}, uint32_t min_byte = 1u,
                                  bool uncut = false, const double spacing[3] = nullptr)
    {
        const double one[3] = {1.0, 1.0, 1.0};
        const double* sp = spacing ? spacing : one;
        std::vector<Surfaced> out;
        std::vector<struct volym_surface_summary> r(1);
        for (const Measured& m : measure(ctx, a, segments, nullptr, uncut, spacing)) {
            volym_surface s{};
            s.box[3] = a.nx; s.box[4] = a.ny; s.box[5] = a.nz;
            s.flags = uncut ? VOLYM_SURFACE_UNCUT : 0u;
            s.min_byte = min_byte;
            s.select[m.label] = 1;
            ctx.check(volym_surface_pass(ctx.handle(), &s));
            ctx.check(volym_read_surface(ctx.handle(), r.data()));
            Surfaced f{};
            f.label = m.label; f.segment = m.segment; f.measured = m.stats.count;
            uint64_t all = 0;
            for (int d = 0; d < 6; ++d) { f.faces[d] = r[0].faces[m.label][d]; f.pairs[d >> 1] += f.faces[d]; all += f.faces[d]; }
            if (all == 0u) continue;
            f.enclosed = r[0].pos[m.label][0] - r[0].neg[m.label][0];
            f.area = static_cast<double>(f.pairs[0]) * sp[1] * sp[2] + static_cast<double>(f.pairs[1]) * sp[0] * sp[2] + static_cast<double>(f.pairs[2]) * sp[0] * sp[1];
            f.volume = static_cast<double>(f.measured) * sp[0] * sp[1] * sp[2];
            f.sphericity = std::cbrt(3.14159265358979323846) * std::pow(6.0 * f.volume, 2.0 / 3.0) / f.area;
            out.push_back(f);
        }
        return out;
    }
    // New: connected components (volym_components_pass) -- is a segment one piece?  Per segment its pieces, its solid texels and the
    // ten largest recorded pieces, largest first (of equals the lowest number); `number` is the piece's id in the id volume.
    struct Piece {
        uint32_t number;
        struct volym_component record;
    };
    struct Pieces {
        uint8_t label;
        std::string segment;
        uint64_t pieces, solid, recorded, small;        // small: recorded pieces of fewer than 8 texels
        std::vector<Piece> top;
    };
    // One components pass per segment, each selected alone as surface selects them, over the scene as it stands (uncut: as it was
    // uploaded).  `segments` as measure takes them.  Segments without a solid texel are left out.
    std::vector<Pieces> components(const GpuContext& ctx, const SimpleAssets& a, const std::vector<std::string>& segments = {}, uint32_t min_byte = 1u,
                                   bool uncut = false)
    {
        std::vector<Pieces> out;
        std::vector<struct volym_components_summary> r(1);
        for (const Measured& m : measure(ctx, a, segments, nullptr, uncut, nullptr)) {
            volym_components q{};
            q.box[3] = a.nx; q.box[4] = a.ny; q.box[5] = a.nz;
            q.flags = uncut ? VOLYM_COMPONENTS_UNCUT : 0u;
            q.min_byte = min_byte;
            q.select[m.label] = 1;
            ctx.check(volym_components_pass(ctx.handle(), &q));
            ctx.check(volym_read_components(ctx.handle(), r.data()));
            if (r[0].n_solid == 0u) continue;
            std::vector<struct volym_component> table(static_cast<size_t>(r[0].recorded));
            ctx.check(volym_read_component_table(ctx.handle(), table.data(), table.size()));
            Pieces p{};
            p.label = m.label; p.segment = m.segment;
            p.pieces = r[0].n_components; p.solid = r[0].n_solid; p.recorded = r[0].recorded;
            std::vector<uint32_t> order(table.size());
            for (size_t k = 0; k < order.size(); ++k) { order[k] = static_cast<uint32_t>(k); if (table[k].count < 8u) ++p.small; }
            const size_t n_top = std::min<size_t>(10, order.size());
            std::partial_sort(order.begin(), order.begin() + n_top, order.end(),
                              [&](uint32_t i, uint32_t j) { return table[i].count != table[j].count ? table[i].count > table[j].count : i < j; });
            for (size_t k = 0; k < n_top; ++k) p.top.push_back(Piece{order[k], table[order[k]]});
            out.push_back(p);
        }
        return out;
    }
    // New: distance maps (volym_distance_pass) -- margins, thickness and clearance.  One distance pass with the union of `segments`
    // selected (empty: every label) over the scene as it stands (uncut: as it was uploaded), weights 1, and the read of its summary;
    // the map stays on the device for volym_read_distance_map and volym_distance_at.  inside: distances to the set's complement
    // (thickness) instead of to the set (margins, clearance).  `nearest`: per label with a present texel at a finite distance, its
    // squared distance to the set and the first texel that attains it.
    struct Nearest {
        uint8_t label;
        std::string segment;
        uint32_t d2, at[3];
    };
    struct Distances {
        struct volym_distance_summary summary;
        bool finite;                            // some texel has a finite distance: max_d2 and max_at mean something
        std::vector<Nearest> nearest;
    };
    Distances distance(const GpuContext& ctx, const SimpleAssets& a, const std::vector<std::string>& segments = {}, bool inside = false, uint32_t min_byte = 1u,
                       bool uncut = false)
    {
        if (!labels_on_device_ && !a.labels_raw.empty()) set_labels(ctx, a);
        volym_distance q{};
        q.box[3] = a.nx; q.box[4] = a.ny; q.box[5] = a.nz;
        q.flags = (uncut ? VOLYM_DISTANCE_UNCUT : 0u) | (inside ? VOLYM_DISTANCE_INSIDE : 0u);
        q.min_byte = min_byte;
        for (int l = 0; l < 256; ++l) q.select[l] = segments.empty() ? 1 : 0;
        for (const std::string& name : segments) q.select[label_value_of(a, name)] = 1;
        q.weight[0] = q.weight[1] = q.weight[2] = 1u;
        ctx.check(volym_distance_pass(ctx.handle(), &q));
        std::vector<Distances> r(1);
        ctx.check(volym_read_distance(ctx.handle(), &r[0].summary));
        r[0].finite = r[0].summary.n_finite != 0u;
        for (int l = 0; l < 256; ++l) {
            if (r[0].summary.near_d2[l] == VOLYM_DISTANCE_NONE) continue;
            Nearest n{static_cast<uint8_t>(l), "label " + std::to_string(l), r[0].summary.near_d2[l],
                      {r[0].summary.near_at[l][0], r[0].summary.near_at[l][1], r[0].summary.near_at[l][2]}};
            for (const SegmentInfo& seg : a.segments) if (seg.label_value == l) { n.segment = seg.name.empty() ? seg.id : seg.name; break; }
            r[0].nearest.push_back(n);
        }
        return r[0];
    }
    // The boundary of the union of `segments` (empty: of every label) as face records in ascending (z, y, x, dir): one surface pass with
    // all of them selected, one emit pass into the context's own buffer, and the read.
    std::vector<struct volym_surface_face> surface_faces(const GpuContext& ctx, const SimpleAssets& a, const std::vector<std::string>& segments = {},
                                                         uint32_t min_byte = 1u, bool uncut = false)
    {
        if (!labels_on_device_ && !a.labels_raw.empty()) set_labels(ctx, a);
        volym_surface s{};
        s.box[3] = a.nx; s.box[4] = a.ny; s.box[5] = a.nz;
        s.flags = uncut ? VOLYM_SURFACE_UNCUT : 0u;
        s.min_byte = min_byte;
        for (int l = 0; l < 256; ++l) s.select[l] = segments.empty() ? 1 : 0;
        for (const std::string& name : segments) s.select[label_value_of(a, name)] = 1;
        ctx.check(volym_surface_pass(ctx.handle(), &s));
        ctx.check(volym_surface_faces_pass(ctx.handle(), nullptr, 0));
        std::vector<struct volym_surface_summary> r(1);
        ctx.check(volym_read_surface(ctx.handle(), r.data()));
        std::vector<struct volym_surface_face> faces(static_cast<size_t>(r[0].total));
        ctx.check(volym_read_surface_faces(ctx.handle(), faces.data(), faces.size()));
        return faces;
    }
    // Binary STL of a face list: 84 + 100 * faces bytes, two triangles per face (corners 0, 1, 2 and 0, 2, 3 of its quad, wound
    // counter-clockwise seen from outside), the normal taken from the face's direction; vertices at origin + texel corner * spacing.
    static void write_stl(const std::string& path, const std::vector<struct volym_surface_face>& faces, const double spacing[3] = nullptr,
                          const double origin[3] = nullptr)
    {
        static const uint8_t corner[6][4][3] = {{{0, 0, 0}, {0, 0, 1}, {0, 1, 1}, {0, 1, 0}}, {{1, 0, 0}, {1, 1, 0}, {1, 1, 1}, {1, 0, 1}},
                                                {{0, 0, 0}, {1, 0, 0}, {1, 0, 1}, {0, 0, 1}}, {{0, 1, 0}, {0, 1, 1}, {1, 1, 1}, {1, 1, 0}},
                                                {{0, 0, 0}, {0, 1, 0}, {1, 1, 0}, {1, 0, 0}}, {{0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}}};
        std::ofstream f(path, std::ios::binary);
        char header[80];
        std::memset(header, ' ', sizeof header);
        std::memcpy(header, "volym segment surface (binary STL)", 34);
        f.write(header, sizeof header);
        const uint32_t n = static_cast<uint32_t>(2u * faces.size());
        f.write(reinterpret_cast<const char*>(&n), 4);
        for (const struct volym_surface_face& face : faces) {
            const uint16_t t[3] = {face.x, face.y, face.z};
            float v[4][3];
            for (int k = 0; k < 4; ++k)
                for (int c = 0; c < 3; ++c)
                    v[k][c] = static_cast<float>((origin ? origin[c] : 0.0) + static_cast<double>(t[c] + corner[face.dir][k][c]) * (spacing ? spacing[c] : 1.0));
            float normal[3] = {0.0f, 0.0f, 0.0f};
            normal[face.dir >> 1] = (face.dir & 1u) ? 1.0f : -1.0f;
            const uint16_t attr = 0;
            static const int triangle[2][3] = {{0, 1, 2}, {0, 2, 3}};
            for (const auto& tri : triangle) {
                f.write(reinterpret_cast<const char*>(normal), 12);
                for (int k = 0; k < 3; ++k) f.write(reinterpret_cast<const char*>(v[tri[k]]), 12);
                f.write(reinterpret_cast<const char*>(&attr), 2);
            }
        }
    }
    // a colour per label value of the segments table for the slice overlay: hues spread by the golden angle over the label values,
    // saturation 0.85, value 1; every other label, 0 included, stays transparent
    static void segment_palette(const SimpleAssets& a, uint8_t strength, uint8_t palette[256][4])
    {
        for (int l = 0; l < 256; ++l) for (int c = 0; c < 4; ++c) palette[l][c] = 0;
        for (const SegmentInfo& seg : a.segments) {
            const uint32_t l = seg.label_value;
            if (l == 0u) continue;
            const double h6 = std::fmod(l * 0.61803398875, 1.0) * 6.0, sat = 0.85;
            const int sector = static_cast<int>(h6) % 6;
            const double f = h6 - std::floor(h6), p = 1.0 - sat, q = 1.0 - sat * f, t = 1.0 - sat * (1.0 - f);
            const double rgb[6][3] = {{1, t, p}, {q, 1, p}, {p, 1, t}, {p, q, 1}, {t, p, 1}, {1, p, q}};
            for (int c = 0; c < 3; ++c) palette[l][c] = static_cast<uint8_t>(rgb[sector][c] * 255.0 + 0.5);
            palette[l][3] = strength;
        }
    }
    static uint32_t crop_texel(float p, uint32_t n)
    {
        const double t = std::floor(static_cast<double>(p) * n + 0.5);
        return t <= 0.0 ? 0u : t >= static_cast<double>(n) ? n : static_cast<uint32_t>(t);
    }
    // src/demos/simple/importance.rs:148-158 as a table: the first segment whose label_value matches wins, the default is 0
    static std::vector<uint8_t> segment_table(const std::vector<SegmentInfo>& segments)
    {
        std::vector<uint8_t> t(256, 0);
        for (size_t i = segments.size(); i-- > 0;) t[segments[i].label_value] = segments[i].importance;
        return t;
    }

private:
    float eye_[3] = {0.0f, 0.0f, 0.0f};
    volym_camera_uniforms camera_{};
    float dense_step_ = 0.0025f;
    bool labels_on_device_ = false;
    bool records_current_ = false;             // the device holds the records of a whole-frame pick pass of the current view and scene
    float records_alpha_min_ = 0.0f;
    std::vector<volym_pick_record> records_host_;   // their host copy, read back by the first highlight_at
};

}  // namespace volym
