// Internal: the seam in front of scene_bytes.hip, for the units that read or edit the scene's bytes through its transition's pieces:
// the measure pass (measure.hip) and the label edits (relabel.hip, brush.hip, lasso.hip, smooth.hip).  Everything else of that unit is static.
#pragma once

#include "context.hpp"
#include "scene_chunks.h"

namespace volym {

struct SceneCut;      // (scene_bytes.hip: the plane a clip edit moves from; no unit but that one has a use for it)

// What follows a change of labels under a (box, plane, mask) that stays, once the labels are stored: the counterpart of retarget.
// `res` names the labels that left and arrived and the hull of the changed texels (changed != 0).  Blocking.
int follow_labels(volym_ctx* c, const volym_relabel_result& res, const char* who);
// a hidden label has voxels (hiding label values no voxel carries changes no byte)
bool mask_active(const volym_ctx* c);
// the uncut copies a cut needs and the context does not hold yet, on slot 0's stream; only while the bytes they copy are uncut
int ensure_uncropped_copies(volym_ctx* c, bool vol);
// the walk over box {lo[3], hi[3]} of a volume in the given layout, cut by the context's crop box and plane; returns its items
uint64_t make_crop_slab(const volym_ctx* c, bool bricked, const uint32_t box[6], const SceneCut* moved_from, CropSlab& s);
// grid of the kernels that stream n_chunks items, one per lane and step: at most eight workgroups per CU, at least one
uint32_t stream_grid(const volym_ctx* c, uint64_t n_chunks);
// the importances have the volume's dimensions: they are cut with it, and an edit carries them along
bool imp_croppable(const volym_ctx* c);

}  // namespace volym
