// The label edit (volym_edit_labels, volym_relabel_check, volym_read_labels): included at the end of scene_bytes.hip, beside the
// kernels it launches (relabel_kernels.h) and the transition whose pieces it is built from (rewrite, ensure_uncropped_copies,
// refresh_macro_cells, scan_label_stats).  A blocking set-up call like the other edits of that unit.

#include <cstddef>

static_assert(sizeof(volym_relabel) == 308 && offsetof(volym_relabel, flags) == 24 && offsetof(volym_relabel, to) == 36 && offsetof(volym_relabel, id_lo) == 292 &&
              offsetof(volym_relabel, d2_lo) == 300, "volym_relabel has no padding");
static_assert(sizeof(volym_relabel_result) == 4128 && offsetof(volym_relabel_result, left) == 8 && offsetof(volym_relabel_result, arrived) == 2056 &&
              offsetof(volym_relabel_result, box) == 4104, "volym_relabel_result has no padding");

// The edit's own transition, the counterpart of retarget for a change of labels under a (box, plane, mask) that stays.
// Precondition: density and importances hold the invariant of context.hpp for the labels as they are.  Postcondition: they hold it
// for the edited labels, label_count and label_box describe those, and everything derived from the bytes is up to date.  With no
// texel changed (or DRY_RUN) nothing but the result is written.  A failure after the kernel has stored leaves bytes that belong to
// neither state: the context then asks for volym_set_volume again, as after a failed retarget.
static int edit_labels(volym_ctx* c, const volym_relabel* r, volym_relabel_result& res)
{
    const bool with_ids = (r->flags & VOLYM_RELABEL_IDS) != 0u, with_map = (r->flags & VOLYM_RELABEL_DISTANCE) != 0u;
    const bool uncut_bytes = (r->flags & VOLYM_RELABEL_UNCUT) != 0u, dry = (r->flags & VOLYM_RELABEL_DRY_RUN) != 0u;
    std::memset(&res, 0, sizeof res);
    for (int a = 0; a < 3; ++a) if (r->box[a] == r->box[3 + a]) return VOLYM_OK;      // an empty box: nothing to walk

    int rc = quiesce_slots(c);
    if (rc != VOLYM_OK) return rc;
    // A hidden label that has voxels has made the uncut copies already; one without voxels has not (retarget takes the idle path for
    // it), and texels are about to move into it.  The bytes are still uncut then: the precondition of ensure_uncropped_copies.
    bool hidden_target = false;
    for (int l = 0; l < 256; ++l) hidden_target = hidden_target || (r->to[l] != l && c->seg_hidden[r->to[l]]);
    if (hidden_target || mask_active(c)) {
        rc = ensure_uncropped_copies(c, true);                            // in stream order in front of the kernel and the rewrites
        if (rc != VOLYM_OK) return rc;
    }

    const hipStream_t stream = c->slot0().stream;
    volym_relabel_result init = {};
    for (int a = 0; a < 3; ++a) init.box[a] = 0xffffffffu;                // lo = max, hi = 0: the kernel keeps INCLUSIVE maxima
    volym_relabel_result* d_res = nullptr;
    hipError_t e = hipMalloc(&d_res, sizeof init);
    if (e != hipSuccess) return fail(c, VOLYM_E_NOMEM, std::string("hipMalloc(relabel result): ") + hipGetErrorString(e));
    e = hipMemcpyAsync(d_res, &init, sizeof init, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) {
        CropSlab s;
        const uint64_t items = make_crop_slab(c, c->bricked, r->box, nullptr, s);
        // keep = inside the request's box, whatever the crop box and the plane are: the cuts are in the bytes the window reads
        for (int a = 0; a < 3; ++a) { s.box_lo[a] = r->box[a]; s.box_hi[a] = r->box[3 + a]; }
        s.planes = 0u; s.pn[0] = s.pn[1] = s.pn[2] = s.pd = 0;
        RelabelRule rule = {};
        rule.min_byte = r->min_byte; rule.max_byte = r->max_byte;
        rule.id_lo = r->id_lo; rule.id_hi = r->id_hi; rule.ids_except = (r->flags & VOLYM_RELABEL_IDS_EXCEPT) ? 1u : 0u;
        rule.d2_lo = r->d2_lo; rule.d2_hi = r->d2_hi;
        rule.store = dry ? 0u : 1u;
        std::memcpy(rule.ids_box, c->component_box, sizeof rule.ids_box);
        std::memcpy(rule.map_box, c->distance_box, sizeof rule.map_box);
        LabelTable to;
        std::memcpy(to.v, r->to, 256);
        const RelabelOut out = {reinterpret_cast<unsigned long long*>(&d_res->changed), reinterpret_cast<unsigned long long*>(d_res->left),
                                reinterpret_cast<unsigned long long*>(d_res->arrived), d_res->box};
        const uint4* vol = reinterpret_cast<const uint4*>(uncut_bytes && c->d_vol0 ? c->d_vol0 : c->d_vol);
        const auto kernel = with_ids ? (with_map ? volym_relabel_kernel<true, true> : volym_relabel_kernel<true, false>)
                                     : (with_map ? volym_relabel_kernel<false, true> : volym_relabel_kernel<false, false>);
        hipLaunchKernelGGL(kernel, dim3(stream_grid(c, items)), dim3(256), 0, stream, reinterpret_cast<uint4*>(c->d_labels), vol,
                           with_ids ? c->component_ids.ptr : nullptr, with_map ? c->distance_map.ptr : nullptr, out, to, s, rule, c->nx, c->ny, c->nz,
                           c->bricked ? 1u : 0u, static_cast<uint32_t>(items));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&res, d_res, sizeof res, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)hipFree(d_res);
    if (e != hipSuccess) {
        std::memset(&res, 0, sizeof res);
        if (!dry) c->have_vol = c->have_frame = false;                    // (the kernel may have stored)
        return fail(c, VOLYM_E_HIP, std::string("volym_edit_labels: ") + hipGetErrorString(e));
    }
    if (res.changed == 0u) { std::memset(res.box, 0, sizeof res.box); return VOLYM_OK; }
    for (int a = 3; a < 6; ++a) ++res.box[a];                             // hi exclusive
    if (dry) return VOLYM_OK;

    const auto work = [&]() -> int {
        // counts and boxes first: mask_active and volym_visibility_boxes read them
        const hipError_t es = scan_label_stats(c);
        if (es != hipSuccess) return fail(c, VOLYM_E_HIP, std::string("volym_edit_labels (label statistics): ") + hipGetErrorString(es));
        ++c->scene_serial;                                                // labels changed: a surface pass is stale
        // A texel's bytes differ from the rule's only where its old and its new label differ in what they give: visibility for the
        // density, visibility and the table's byte for importances mapped from the labels.  Every such texel carries a label that
        // arrived, inside the result's box: the visibility kernel stores the chunks that hold one, whole, by the rule.
        uint8_t flipped[256];
        bool hidden_moved = false;
        for (int l = 0; l < 256; ++l) {
            flipped[l] = res.left[l] != 0u || res.arrived[l] != 0u;
            hidden_moved = hidden_moved || (flipped[l] && c->seg_hidden[l]);
        }
        int rc = VOLYM_OK;
        if (hidden_moved) rc = rewrite(c, density_of(c), res.box, flipped, nullptr);
        if (rc == VOLYM_OK && imp_croppable(c) && (imp_from_labels(c) || hidden_moved)) rc = rewrite(c, importances_of(c), res.box, flipped, nullptr);
        if (rc == VOLYM_OK && hidden_moved) rc = refresh_macro_cells(c, &res.box, 1u);
        if (rc != VOLYM_OK) return rc;
        HIPCHK(c, hipStreamSynchronize(c->slot0().stream));               // every slot's next frame reads the new bytes
        if (imp_from_labels(c)) segment_important_box(c);
        crop_important_box(c);
        return rebuild_lists(c);
    };
    rc = work();
    if (rc != VOLYM_OK) c->have_vol = c->have_frame = false;
    return rc;
}

extern "C" {

int volym_relabel_check(const volym_relabel* r, const uint32_t dims[3])
{
    if (!r || !dims) return VOLYM_E_INVALID;
    if (!box_in_volume(r->box, dims)) return VOLYM_E_INVALID;
    const uint32_t known = VOLYM_RELABEL_UNCUT | VOLYM_RELABEL_IDS | VOLYM_RELABEL_IDS_EXCEPT | VOLYM_RELABEL_DISTANCE | VOLYM_RELABEL_DRY_RUN;
    if (r->flags & ~known) return VOLYM_E_INVALID;
    if ((r->flags & VOLYM_RELABEL_IDS_EXCEPT) && !(r->flags & VOLYM_RELABEL_IDS)) return VOLYM_E_INVALID;
    if (r->min_byte > r->max_byte || r->max_byte > 255u) return VOLYM_E_INVALID;
    if ((r->flags & VOLYM_RELABEL_IDS) && r->id_lo > r->id_hi) return VOLYM_E_INVALID;
    if ((r->flags & VOLYM_RELABEL_DISTANCE) && r->d2_lo > r->d2_hi) return VOLYM_E_INVALID;
    return VOLYM_OK;
}

int volym_edit_labels(volym_ctx* c, const volym_relabel* r, struct volym_relabel_result* out)
{
    if (!c) return VOLYM_E_INVALID;
    if (!r) return fail(c, VOLYM_E_INVALID, "volym_edit_labels: NULL request");
    if (!c->have_vol) return fail(c, VOLYM_E_STATE, "volym_edit_labels: no volume (volym_set_volume first)");
    if (!labels_fit(c)) return fail(c, VOLYM_E_STATE, "volym_edit_labels: no labels of the volume's dimensions (volym_set_labels first; volym_set_importances drops them)");
    if (c->labels_bricked != c->bricked || (imp_croppable(c) && c->imp_bricked != c->labels_bricked))
        return fail(c, VOLYM_E_STATE, "volym_edit_labels: volume, importances and labels were uploaded under different VOLYM_OPT_VOLUME_LAYOUT settings");
    const uint32_t dims[3] = {c->nx, c->ny, c->nz};
    if (volym_relabel_check(r, dims) != VOLYM_OK)
        return fail(c, VOLYM_E_INVALID, "volym_edit_labels: need lo <= hi <= volume size on every axis, known flags, IDS_EXCEPT only with IDS, min_byte <= max_byte <= 255, "
                                        "id_lo <= id_hi with IDS and d2_lo <= d2_hi with DISTANCE");
    const auto inside = [&](const uint32_t box[6]) {
        for (int a = 0; a < 3; ++a) if (r->box[a] < box[a] || r->box[3 + a] > box[3 + a]) return false;
        return true;
    };
    if (r->flags & VOLYM_RELABEL_IDS) {
        if (c->components.count == 0u) return fail(c, VOLYM_E_STATE, "volym_edit_labels: IDS without a volym_components_pass since the volume was set");
        if (!inside(c->component_box)) return fail(c, VOLYM_E_INVALID, "volym_edit_labels: IDS with a box that reaches outside the box of the components pass");
    }
    if (r->flags & VOLYM_RELABEL_DISTANCE) {
        if (c->distance.count == 0u) return fail(c, VOLYM_E_STATE, "volym_edit_labels: DISTANCE without a volym_distance_pass since the volume was set");
        if (!inside(c->distance_box)) return fail(c, VOLYM_E_INVALID, "volym_edit_labels: DISTANCE with a box that reaches outside the box of the distance pass");
    }
    HIPCHK(c, hipSetDevice(c->device));
    volym_relabel_result res;
    const int rc = edit_labels(c, r, res);
    if (rc == VOLYM_OK && out) *out = res;
    return rc;
}

int volym_read_labels(volym_ctx* c, const uint32_t sub[6], uint8_t* out)
{
    if (!c) return VOLYM_E_INVALID;
    if (!c->d_labels) return fail(c, VOLYM_E_STATE, "volym_read_labels: no labels (volym_set_labels first; volym_set_importances drops them)");
    const uint32_t dims[3] = {c->lnx, c->lny, c->lnz};
    uint32_t whole[6];
    whole_volume_box(dims, whole);
    if (!sub) sub = whole;
    if (!box_in_volume(sub, dims)) return fail(c, VOLYM_E_INVALID, "volym_read_labels: the sub-box must have lo <= hi <= the labels' dimensions on every axis");
    const uint32_t w = sub[3] - sub[0], h = sub[4] - sub[1];
    const uint64_t total = static_cast<uint64_t>(w) * h * (sub[5] - sub[2]);
    if (total == 0u) return VOLYM_OK;
    if (!out) return fail(c, VOLYM_E_INVALID, "volym_read_labels: NULL output");
    HIPCHK(c, hipSetDevice(c->device));
    const hipStream_t stream = c->slot0().stream;
    uint8_t* d_out = nullptr;
    hipError_t e = hipMalloc(&d_out, total);
    if (e != hipSuccess) return fail(c, VOLYM_E_NOMEM, std::string("hipMalloc(label read-back): ") + hipGetErrorString(e));
    hipLaunchKernelGGL(volym_read_labels_kernel, dim3(static_cast<uint32_t>((total + 255u) / 256u)), dim3(256), 0, stream, c->d_labels, d_out, c->lnx, c->lny,
                       c->labels_bricked ? 1u : 0u, sub[0], sub[1], sub[2], w, h, total);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, total, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)hipFree(d_out);
    if (e != hipSuccess) return fail(c, VOLYM_E_HIP, std::string("volym_read_labels: ") + hipGetErrorString(e));
    return VOLYM_OK;
}

}  // extern "C"
