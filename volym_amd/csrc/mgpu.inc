// Native multi-GPU frame loop (include/volym_mgpu.h).  Included at the end of raymarch.hip: it launches the same kernels.
//
// Per frame i, rotating buffer b = i % NBUF, on every local device:
//   march stream:  wait(buffer b free) -> ray-march of the rank's tiles -> pack (only the tiles that are not constant) -> event
//   comm stream:   wait(packed) -> ncclSend to the root            (root: ncclRecv from every peer, all in one group)
//                  root: assemble the raster from the gathered packed shards -> event(buffer b free)
// so the collective and the assemble of frame i run beside the marches of frames i+1 .. i+NBUF-1.
#include <dlfcn.h>
#include <rccl/rccl.h>

#include "../../include/volym_mgpu.h"

namespace {

constexpr int MG_NBUF = 4;

struct RcclApi {
    void* handle = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
};

RcclApi g_rccl;
std::mutex g_rccl_mu;

// RCCL on first use: the library the process already has (torch ships its own librccl.so.1) or the ROCm one
bool rccl_load(std::string& err)
{
    std::lock_guard<std::mutex> lk(g_rccl_mu);
    if (g_rccl.handle) return true;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void* h = nullptr;
    for (const char* n : names) { h = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (h) break; }
    if (!h) { err = std::string("cannot load RCCL (librccl.so.1): ") + (dlerror() ? dlerror() : "?"); return false; }
#define VOLYM_RCCL_SYM(field, name)                                                              \
    g_rccl.field = reinterpret_cast<decltype(g_rccl.field)>(dlsym(h, name));                     \
    if (!g_rccl.field) { err = std::string("RCCL lacks ") + name; dlclose(h); return false; }
    VOLYM_RCCL_SYM(GetUniqueId, "ncclGetUniqueId")
    VOLYM_RCCL_SYM(CommInitRank, "ncclCommInitRank")
    VOLYM_RCCL_SYM(CommInitAll, "ncclCommInitAll")
    VOLYM_RCCL_SYM(CommDestroy, "ncclCommDestroy")
    VOLYM_RCCL_SYM(GroupStart, "ncclGroupStart")
    VOLYM_RCCL_SYM(GroupEnd, "ncclGroupEnd")
    VOLYM_RCCL_SYM(Send, "ncclSend")
    VOLYM_RCCL_SYM(Recv, "ncclRecv")
    VOLYM_RCCL_SYM(AllReduce, "ncclAllReduce")
    VOLYM_RCCL_SYM(GetErrorString, "ncclGetErrorString")
#undef VOLYM_RCCL_SYM
    g_rccl.handle = h;
    return true;
}

struct MgLocal {
    int device = 0;
    int rank = 0;
    volym_ctx* ctx = nullptr;
    hipStream_t s_comm = nullptr;
    ncclComm_t comm = nullptr;
    uint8_t* packed[MG_NBUF] = {};      // this rank's packed shard of the frames in flight (root: inside gathered[b])
    bool owns_packed = false;
    hipEvent_t ev_packed[MG_NBUF] = {}; // march stream: shard b packed
    hipEvent_t ev_free[MG_NBUF] = {};   // buffer b may be packed into again
    bool free_pending[MG_NBUF] = {};    // ev_free[b] has been recorded (outside a capture)
    uint32_t* d_scalar = nullptr;
};

thread_local std::string g_mg_create_error;

}  // namespace

struct volym_mgpu {
    uint32_t W = 0, H = 0;
    int world = 1;
    int transport = VOLYM_MGPU_RCCL;
    bool multi_process = false;
    std::vector<MgLocal> loc;
    int root = -1;                       // index into loc of rank 0, or -1 in a process that does not hold it
    uint8_t* gathered[MG_NBUF] = {};     // root device: world packed shards, msg_bytes apart
    hipEvent_t ev_gathered[MG_NBUF] = {};   // COPY transport: every peer's shard b has been copied to the root
    size_t msg_bytes = 0;
    bool prepared = false;
    uint64_t frame_no = 0;
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    hipEvent_t ev_fork = nullptr;        // graph capture over several local ranks (one device): fork / join of their streams
    std::vector<hipEvent_t> ev_join;
    uint64_t graph_view = 0;
    std::string err;
};

namespace {

int mg_fail(volym_mgpu* m, int code, const std::string& msg)
{
    if (m) m->err = msg; else g_mg_create_error = msg;
    return code;
}

#define MG_HIP(m, expr)                                                                                   \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return mg_fail(m, VOLYM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
#define MG_NCCL(m, expr)                                                                                  \
    do {                                                                                                  \
        ncclResult_t r_ = (expr);                                                                         \
        if (r_ != ncclSuccess) return mg_fail(m, VOLYM_E_HIP, std::string(#expr) + ": " + g_rccl.GetErrorString(r_)); \
    } while (0)
#define MG_CTX(m, L, expr)                                                                                \
    do {                                                                                                  \
        int rc_ = (expr);                                                                                 \
        if (rc_ != VOLYM_OK) return mg_fail(m, rc_, std::string("rank ") + std::to_string((L).rank) + ": " + volym_last_error((L).ctx)); \
    } while (0)

int mg_make_local(volym_mgpu* m, MgLocal& L, int device, int rank)
{
    L.device = device;
    L.rank = rank;
    int rc = volym_create(&L.ctx, m->W, m->H, device);
    if (rc != VOLYM_OK) return mg_fail(m, rc, std::string("volym_create: ") + volym_last_error(nullptr));
    MG_CTX(m, L, volym_set_shard(L.ctx, static_cast<uint32_t>(rank), static_cast<uint32_t>(m->world)));
    MG_HIP(m, hipSetDevice(device));
    MG_HIP(m, hipStreamCreateWithFlags(&L.s_comm, hipStreamNonBlocking));
    for (int b = 0; b < MG_NBUF; ++b) {
        MG_HIP(m, hipEventCreateWithFlags(&L.ev_packed[b], hipEventDisableTiming));
        MG_HIP(m, hipEventCreateWithFlags(&L.ev_free[b], hipEventDisableTiming));
    }
    MG_HIP(m, hipMalloc(&L.d_scalar, 64));
    return VOLYM_OK;
}

void mg_free_buffers(volym_mgpu* m)
{
    for (MgLocal& L : m->loc) {
        (void)hipSetDevice(L.device);
        if (L.ctx) (void)volym_sync(L.ctx);
        if (L.s_comm) (void)hipStreamSynchronize(L.s_comm);
        for (int b = 0; b < MG_NBUF; ++b) {
            if (L.owns_packed && L.packed[b]) (void)hipFree(L.packed[b]);
            L.packed[b] = nullptr;
            L.free_pending[b] = false;
        }
        L.owns_packed = false;
    }
    if (m->root >= 0) {
        (void)hipSetDevice(m->loc[m->root].device);
        for (int b = 0; b < MG_NBUF; ++b) { if (m->gathered[b]) (void)hipFree(m->gathered[b]); m->gathered[b] = nullptr; }
    }
    if (m->graph_exec) { (void)hipGraphExecDestroy(m->graph_exec); m->graph_exec = nullptr; }
    if (m->graph) { (void)hipGraphDestroy(m->graph); m->graph = nullptr; }
    m->prepared = false;
}

// Enqueue frame `i` on every local device.  capturing: inside a stream capture (events recorded before the capture are not
// waited on: a replay starts with every buffer free, because replays are ordered on the march stream).
int mg_enqueue_frame(volym_mgpu* m, uint64_t i, bool capturing, bool fresh_cycle)
{
    const int b = static_cast<int>(i % MG_NBUF);
    const size_t msg = m->msg_bytes;
    if (m->world == 1) {                     // nothing to gather: the march writes the raster itself
        MgLocal& L = m->loc[0];
        MG_HIP(m, hipSetDevice(L.device));
        MG_CTX(m, L, ctx_launch_march(L.ctx));
        return VOLYM_OK;
    }
    for (MgLocal& L : m->loc) {
        MG_HIP(m, hipSetDevice(L.device));
        hipStream_t s_march = L.ctx->slot0().stream;
        if (L.free_pending[b] && !(capturing && fresh_cycle)) MG_HIP(m, hipStreamWaitEvent(s_march, L.ev_free[b], 0));
        MG_CTX(m, L, ctx_launch_march(L.ctx));
        MG_CTX(m, L, volym_pack_shard(L.ctx, L.packed[b], msg));
        MG_HIP(m, hipEventRecord(L.ev_packed[b], s_march));
        MG_HIP(m, hipStreamWaitEvent(L.s_comm, L.ev_packed[b], 0));
    }
    MgLocal* R = m->root >= 0 ? &m->loc[m->root] : nullptr;
    if (m->world > 1) {
        if (m->transport == VOLYM_MGPU_RCCL) {
            // rooted gather as grouped point-to-point transfers: every peer sends straight to the root
            // (an error inside the group closes the group before it is reported: a group left open would swallow the next call)
            MG_NCCL(m, g_rccl.GroupStart());
            ncclResult_t gr = ncclSuccess;
            for (MgLocal& L : m->loc)
                if (L.rank != 0 && gr == ncclSuccess) gr = g_rccl.Send(L.packed[b], msg, ncclUint8, 0, L.comm, L.s_comm);
            if (R)
                for (int r = 1; r < m->world && gr == ncclSuccess; ++r)
                    gr = g_rccl.Recv(m->gathered[b] + static_cast<size_t>(r) * msg, msg, ncclUint8, r, R->comm, R->s_comm);
            const ncclResult_t ge = g_rccl.GroupEnd();
            MG_NCCL(m, gr);
            MG_NCCL(m, ge);
        } else {
            // one process: the root pulls the peers' shards (peer copies; same-device copies for virtual ranks)
            MG_HIP(m, hipSetDevice(R->device));
            for (MgLocal& L : m->loc) {
                if (L.rank == 0) continue;
                MG_HIP(m, hipStreamWaitEvent(R->s_comm, L.ev_packed[b], 0));
                if (L.device == R->device)
                    MG_HIP(m, hipMemcpyAsync(m->gathered[b] + static_cast<size_t>(L.rank) * msg, L.packed[b], msg, hipMemcpyDeviceToDevice, R->s_comm));
                else
                    MG_HIP(m, hipMemcpyPeerAsync(m->gathered[b] + static_cast<size_t>(L.rank) * msg, R->device, L.packed[b], L.device, msg, R->s_comm));
            }
            MG_HIP(m, hipEventRecord(m->ev_gathered[b], R->s_comm));
        }
    }
    if (R) {
        MG_HIP(m, hipSetDevice(R->device));
        volym_ctx* c = R->ctx;
        hipLaunchKernelGGL(volym_assemble_packed_kernel, dim3(c->n_tiles), dim3(256), 0, R->s_comm, m->gathered[b], msg, c->frame_buf(c->slot0()), c->W, c->H,
                           c->tiles_x, c->n_tiles, c->world, c->shard_tiles);
        MG_HIP(m, hipGetLastError());
    }
    for (MgLocal& L : m->loc) {
        MG_HIP(m, hipSetDevice(L.device));
        if (L.rank == 0 || m->transport == VOLYM_MGPU_RCCL || m->world == 1) {
            MG_HIP(m, hipEventRecord(L.ev_free[b], L.s_comm));          // after its send / after the root's assemble
        } else {
            // COPY transport: the peer's buffer is free once the root's copies are through
            MG_HIP(m, hipStreamWaitEvent(L.s_comm, m->ev_gathered[b], 0));
            MG_HIP(m, hipEventRecord(L.ev_free[b], L.s_comm));
        }
        if (!capturing) L.free_pending[b] = true;
    }
    return VOLYM_OK;
}

int mg_drain(volym_mgpu* m)
{
    for (MgLocal& L : m->loc) {
        MG_HIP(m, hipSetDevice(L.device));
        MG_HIP(m, hipStreamSynchronize(L.ctx->slot0().stream));
        MG_HIP(m, hipStreamSynchronize(L.s_comm));
    }
    return VOLYM_OK;
}

int mg_finish_create(volym_mgpu* m, volym_mgpu** out)
{
    for (size_t i = 0; i < m->loc.size(); ++i) if (m->loc[i].rank == 0) m->root = static_cast<int>(i);
    if (m->root >= 0) {
        (void)hipSetDevice(m->loc[m->root].device);
        for (int b = 0; b < MG_NBUF; ++b)
            if (hipEventCreateWithFlags(&m->ev_gathered[b], hipEventDisableTiming) != hipSuccess) return mg_fail(m, VOLYM_E_HIP, "hipEventCreate failed");
    }
    *out = m;
    return VOLYM_OK;
}

}  // namespace

extern "C" {

const char* volym_mgpu_last_error(const volym_mgpu* m) { return m ? m->err.c_str() : g_mg_create_error.c_str(); }

int volym_mgpu_unique_id(uint8_t id[128])
{
    if (!id) return VOLYM_E_INVALID;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    std::string err;
    if (!rccl_load(err)) return mg_fail(nullptr, VOLYM_E_STATE, err);
    ncclUniqueId u;
    ncclResult_t r = g_rccl.GetUniqueId(&u);
    if (r != ncclSuccess) return mg_fail(nullptr, VOLYM_E_HIP, std::string("ncclGetUniqueId: ") + g_rccl.GetErrorString(r));
    std::memcpy(id, &u, 128);
    return VOLYM_OK;
}

void volym_mgpu_destroy(volym_mgpu* m)
{
    if (!m) return;
    mg_free_buffers(m);
    for (MgLocal& L : m->loc) {
        (void)hipSetDevice(L.device);
        if (L.comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(L.comm);
        for (int b = 0; b < MG_NBUF; ++b) {
            if (L.ev_packed[b]) (void)hipEventDestroy(L.ev_packed[b]);
            if (L.ev_free[b]) (void)hipEventDestroy(L.ev_free[b]);
        }
        if (L.d_scalar) (void)hipFree(L.d_scalar);
        if (L.s_comm) (void)hipStreamDestroy(L.s_comm);
        if (L.ctx) volym_destroy(L.ctx);
    }
    for (int b = 0; b < MG_NBUF; ++b) if (m->ev_gathered[b]) (void)hipEventDestroy(m->ev_gathered[b]);
    if (m->ev_fork) (void)hipEventDestroy(m->ev_fork);
    for (hipEvent_t e : m->ev_join) if (e) (void)hipEventDestroy(e);
    delete m;
}

int volym_mgpu_create(volym_mgpu** out, uint32_t width, uint32_t height, int n_devices, const int* device_ids, int transport)
{
    if (!out) return mg_fail(nullptr, VOLYM_E_INVALID, "volym_mgpu_create: out is NULL");
    *out = nullptr;
    if (n_devices < 1 || n_devices > 64 || !device_ids) return mg_fail(nullptr, VOLYM_E_INVALID, "volym_mgpu_create: 1..64 devices");
    if (transport != VOLYM_MGPU_RCCL && transport != VOLYM_MGPU_COPY) return mg_fail(nullptr, VOLYM_E_INVALID, "volym_mgpu_create: unknown transport");
    if (transport == VOLYM_MGPU_RCCL)
        for (int i = 0; i < n_devices; ++i)
            for (int j = 0; j < i; ++j)
                if (device_ids[i] == device_ids[j]) return mg_fail(nullptr, VOLYM_E_INVALID, "volym_mgpu_create: RCCL needs distinct devices (virtual ranks on one device: VOLYM_MGPU_COPY)");
    volym_mgpu* m = new (std::nothrow) volym_mgpu();
    if (!m) return mg_fail(nullptr, VOLYM_E_NOMEM, "out of host memory");
    m->W = width; m->H = height; m->world = n_devices; m->transport = transport; m->multi_process = false;
    m->loc.resize(static_cast<size_t>(n_devices));
    for (int i = 0; i < n_devices; ++i) {
        int rc = mg_make_local(m, m->loc[static_cast<size_t>(i)], device_ids[i], i);
        if (rc != VOLYM_OK) { g_mg_create_error = m->err; volym_mgpu_destroy(m); return rc; }
    }
    if (transport == VOLYM_MGPU_RCCL && n_devices > 1) {
        std::string err;
        if (!rccl_load(err)) { volym_mgpu_destroy(m); return mg_fail(nullptr, VOLYM_E_STATE, err); }
        std::vector<ncclComm_t> comms(static_cast<size_t>(n_devices));
        ncclResult_t r = g_rccl.CommInitAll(comms.data(), n_devices, device_ids);
        if (r != ncclSuccess) { volym_mgpu_destroy(m); return mg_fail(nullptr, VOLYM_E_HIP, std::string("ncclCommInitAll: ") + g_rccl.GetErrorString(r)); }
        for (int i = 0; i < n_devices; ++i) m->loc[static_cast<size_t>(i)].comm = comms[static_cast<size_t>(i)];
    }
    if (transport == VOLYM_MGPU_COPY)
        for (int i = 1; i < n_devices; ++i)
            if (device_ids[i] != device_ids[0]) { (void)hipSetDevice(device_ids[0]); (void)hipDeviceEnablePeerAccess(device_ids[i], 0); (void)hipGetLastError(); }
    int rc = mg_finish_create(m, out);
    if (rc != VOLYM_OK) { g_mg_create_error = m->err; volym_mgpu_destroy(m); }
    return rc;
}

int volym_mgpu_create_rank(volym_mgpu** out, uint32_t width, uint32_t height, int device_id, int rank, int world, const uint8_t id[128])
{
    if (!out) return mg_fail(nullptr, VOLYM_E_INVALID, "volym_mgpu_create_rank: out is NULL");
    *out = nullptr;
    if (world < 1 || world > 4096 || rank < 0 || rank >= world) return mg_fail(nullptr, VOLYM_E_INVALID, "volym_mgpu_create_rank: need 0 <= rank < world <= 4096");
    if (world > 1 && !id) return mg_fail(nullptr, VOLYM_E_INVALID, "volym_mgpu_create_rank: the unique id is NULL");
    if (id) { bool all_zero = true; for (int i = 0; i < 128; ++i) all_zero = all_zero && id[i] == 0; if (all_zero && world == 1) id = nullptr; }
    volym_mgpu* m = new (std::nothrow) volym_mgpu();
    if (!m) return mg_fail(nullptr, VOLYM_E_NOMEM, "out of host memory");
    m->W = width; m->H = height; m->world = world; m->transport = VOLYM_MGPU_RCCL; m->multi_process = true;
    m->loc.resize(1);
    int rc = mg_make_local(m, m->loc[0], device_id, rank);
    if (rc != VOLYM_OK) { g_mg_create_error = m->err; volym_mgpu_destroy(m); return rc; }
    if (id) {                                // (a one-rank communicator too: the same calls as with peers)
        std::string err;
        if (!rccl_load(err)) { volym_mgpu_destroy(m); return mg_fail(nullptr, VOLYM_E_STATE, err); }
        ncclUniqueId u;
        std::memcpy(&u, id, 128);
        (void)hipSetDevice(m->loc[0].device);
        ncclResult_t r = g_rccl.CommInitRank(&m->loc[0].comm, world, u, rank);
        if (r != ncclSuccess) { volym_mgpu_destroy(m); return mg_fail(nullptr, VOLYM_E_HIP, std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(r)); }
    }
    rc = mg_finish_create(m, out);
    if (rc != VOLYM_OK) { g_mg_create_error = m->err; volym_mgpu_destroy(m); }
    return rc;
}

int volym_mgpu_world(const volym_mgpu* m) { return m ? m->world : 0; }
int volym_mgpu_local_count(const volym_mgpu* m) { return m ? static_cast<int>(m->loc.size()) : 0; }
volym_ctx* volym_mgpu_context(volym_mgpu* m, int i) { return (m && i >= 0 && i < static_cast<int>(m->loc.size())) ? m->loc[static_cast<size_t>(i)].ctx : nullptr; }
int volym_mgpu_local_rank(const volym_mgpu* m, int i) { return (m && i >= 0 && i < static_cast<int>(m->loc.size())) ? m->loc[static_cast<size_t>(i)].rank : -1; }

// A captured loop carries the frame parameters, culling buffers and distance fields of the scene it was captured for, and is
// keyed on the view alone: a set-up call that changes the scene (at a standing view too) makes the next volym_mgpu_run capture again.
static void mg_drop_graph(volym_mgpu* m) { m->graph_view = 0; }

int volym_mgpu_set_volume(volym_mgpu* m, const uint8_t* voxels, uint32_t nx, uint32_t ny, uint32_t nz, int filter)
{
    if (!m) return VOLYM_E_INVALID;
    mg_drop_graph(m);
    for (MgLocal& L : m->loc) MG_CTX(m, L, volym_set_volume(L.ctx, voxels, nx, ny, nz, filter));
    return VOLYM_OK;
}

int volym_mgpu_set_importances(volym_mgpu* m, const uint8_t* importances, uint32_t nx, uint32_t ny, uint32_t nz)
{
    if (!m) return VOLYM_E_INVALID;
    mg_drop_graph(m);
    for (MgLocal& L : m->loc) MG_CTX(m, L, volym_set_importances(L.ctx, importances, nx, ny, nz));
    return VOLYM_OK;
}

int volym_mgpu_set_labels(volym_mgpu* m, const uint8_t* labels, uint32_t nx, uint32_t ny, uint32_t nz)
{
    if (!m) return VOLYM_E_INVALID;
    for (MgLocal& L : m->loc) MG_CTX(m, L, volym_set_labels(L.ctx, labels, nx, ny, nz));
    return VOLYM_OK;
}

int volym_mgpu_set_segment_importances(volym_mgpu* m, const uint8_t table[256])
{
    if (!m) return VOLYM_E_INVALID;
    mg_drop_graph(m);
    for (MgLocal& L : m->loc) MG_CTX(m, L, volym_set_segment_importances(L.ctx, table));
    return VOLYM_OK;
}

int volym_mgpu_set_crop_box(volym_mgpu* m, const uint32_t lo[3], const uint32_t hi[3])
{
    if (!m) return VOLYM_E_INVALID;
    mg_drop_graph(m);
    for (MgLocal& L : m->loc) MG_CTX(m, L, volym_set_crop_box(L.ctx, lo, hi));
    return VOLYM_OK;
}

int volym_mgpu_set_clip_plane(volym_mgpu* m, const int32_t n[3], int32_t d)
{
    if (!m) return VOLYM_E_INVALID;
    mg_drop_graph(m);
    for (MgLocal& L : m->loc) MG_CTX(m, L, volym_set_clip_plane(L.ctx, n, d));
    return VOLYM_OK;
}

int volym_mgpu_set_segment_visibility(volym_mgpu* m, const uint8_t visible[256])
{
    if (!m) return VOLYM_E_INVALID;
    mg_drop_graph(m);
    for (MgLocal& L : m->loc) MG_CTX(m, L, volym_set_segment_visibility(L.ctx, visible));
    return VOLYM_OK;
}

int volym_mgpu_set_transfer_function(volym_mgpu* m, const uint8_t* rgba8, uint32_t n)
{
    if (!m) return VOLYM_E_INVALID;
    mg_drop_graph(m);
    for (MgLocal& L : m->loc) MG_CTX(m, L, volym_set_transfer_function(L.ctx, rgba8, n));
    return VOLYM_OK;
}

int volym_mgpu_set_option(volym_mgpu* m, int key, int value)
{
    if (!m) return VOLYM_E_INVALID;
    // the loop marches a rank's frames on one stream and packs from one shard buffer (DESIGN.md 12.5a): one frame slot per rank here
    if (key == VOLYM_OPT_FRAMES_IN_FLIGHT && value != 1) return mg_fail(m, VOLYM_E_STATE, "volym_mgpu_set_option: VOLYM_OPT_FRAMES_IN_FLIGHT > 1 is not available in the multi-GPU loop");
    for (MgLocal& L : m->loc) MG_CTX(m, L, volym_set_option(L.ctx, key, value));
    return VOLYM_OK;
}

int volym_mgpu_update(volym_mgpu* m, const volym_camera_uniforms* camera, const volym_parameter_uniforms* parameters)
{
    if (!m) return VOLYM_E_INVALID;
    for (MgLocal& L : m->loc) MG_CTX(m, L, volym_update(L.ctx, camera, parameters));
    return VOLYM_OK;
}

int volym_mgpu_prepare(volym_mgpu* m, uint32_t slack_percent)
{
    if (!m) return VOLYM_E_INVALID;
    mg_free_buffers(m);
    if (m->world == 1) {                     // one rank: the march writes the raster, nothing is packed or gathered
        MgLocal& L = m->loc[0];
        if (!L.ctx->have_frame) return mg_fail(m, VOLYM_E_STATE, "volym_mgpu_prepare: call volym_mgpu_update first");
        if (L.comm) {                        // a one-rank communicator still answers its collectives
            uint32_t one = 1;
            MG_HIP(m, hipSetDevice(L.device));
            MG_HIP(m, hipMemcpy(L.d_scalar, &one, sizeof one, hipMemcpyHostToDevice));
            MG_NCCL(m, g_rccl.AllReduce(L.d_scalar, L.d_scalar, 1, ncclUint32, ncclMax, L.comm, L.s_comm));
            MG_HIP(m, hipStreamSynchronize(L.s_comm));
        }
        m->msg_bytes = 0;
        m->prepared = true;
        m->frame_no = 0;
        return VOLYM_OK;
    }
    // one untimed frame per rank, packed with room for every tile: how many tiles does a shard really store?
    // A rank whose probe fails still enters the all-reduce below (with the value 0xffffffff): every rank then fails together
    // instead of leaving its peers inside a collective.
    uint32_t max_used = 0;
    int probe_rc = VOLYM_OK;
    std::string probe_err;
    for (MgLocal& L : m->loc) {
        int rc = VOLYM_OK;
        uint8_t* probe = nullptr;
        if (hipSetDevice(L.device) != hipSuccess) rc = VOLYM_E_HIP;
        if (rc == VOLYM_OK && !L.ctx->have_frame) { rc = VOLYM_E_STATE; probe_err = "volym_mgpu_prepare: call volym_mgpu_update first"; }
        const size_t cap = volym_packed_shard_bytes(L.ctx, 1u << 30);
        if (rc == VOLYM_OK && hipMalloc(&probe, cap) != hipSuccess) { rc = VOLYM_E_NOMEM; probe_err = "volym_mgpu_prepare: hipMalloc(probe)"; }
        // the overflow flag of an earlier preparation must not outlive it (the slots are sized anew below)
        if (rc == VOLYM_OK && hipMemsetAsync(L.ctx->slot0().d_pack_counters + 2, 0, sizeof(uint32_t), L.ctx->slot0().stream) != hipSuccess) rc = VOLYM_E_HIP;
        if (rc == VOLYM_OK) rc = volym_compute_pass(L.ctx);
        if (rc == VOLYM_OK) rc = volym_pack_shard(L.ctx, probe, cap);
        uint32_t used = 0, over = 0;
        if (rc == VOLYM_OK) rc = volym_packed_tiles(L.ctx, &used, &over);
        if (probe) (void)hipFree(probe);
        if (rc != VOLYM_OK && probe_rc == VOLYM_OK) {
            probe_rc = rc;
            if (probe_err.empty()) probe_err = std::string("rank ") + std::to_string(L.rank) + ": " + volym_last_error(L.ctx);
        }
        max_used = std::max(max_used, used);
    }
    if (probe_rc != VOLYM_OK) max_used = 0xffffffffu;
    if (m->multi_process && m->world > 1) {
        MgLocal& L = m->loc[0];
        MG_HIP(m, hipSetDevice(L.device));
        MG_HIP(m, hipMemcpy(L.d_scalar, &max_used, sizeof(uint32_t), hipMemcpyHostToDevice));
        MG_NCCL(m, g_rccl.AllReduce(L.d_scalar, L.d_scalar, 1, ncclUint32, ncclMax, L.comm, L.s_comm));
        MG_HIP(m, hipStreamSynchronize(L.s_comm));
        MG_HIP(m, hipMemcpy(&max_used, L.d_scalar, sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    if (probe_rc != VOLYM_OK) return mg_fail(m, probe_rc, probe_err);
    if (max_used == 0xffffffffu) return mg_fail(m, VOLYM_E_STATE, "volym_mgpu_prepare: another rank failed to render its probe frame");
    const volym_ctx* c0 = m->loc[0].ctx;
    const uint64_t want = static_cast<uint64_t>(max_used) * (100u + std::min(slack_percent, 1000u)) / 100u + (slack_percent ? 8u : 0u);
    const uint32_t tiles = static_cast<uint32_t>(std::min<uint64_t>(want, c0->shard_tiles));
    m->msg_bytes = volym_packed_shard_bytes(c0, tiles);
    if (m->root >= 0) {
        MG_HIP(m, hipSetDevice(m->loc[m->root].device));
        for (int b = 0; b < MG_NBUF; ++b) MG_HIP(m, hipMalloc(&m->gathered[b], m->msg_bytes * static_cast<size_t>(m->world)));
    }
    for (MgLocal& L : m->loc) {
        MG_HIP(m, hipSetDevice(L.device));
        for (int b = 0; b < MG_NBUF && m->world > 1; ++b) {
            if (L.rank == 0) { L.packed[b] = m->gathered[b]; }            // the root packs straight into its slot of the gathered buffer
            else { MG_HIP(m, hipMalloc(&L.packed[b], m->msg_bytes)); L.owns_packed = true; }
        }
    }
    m->prepared = true;
    m->frame_no = 0;
    return VOLYM_OK;
}

int volym_mgpu_run(volym_mgpu* m, uint32_t frames, int use_graph, volym_mgpu_timing* timing)
{
    if (!m || frames == 0) return VOLYM_E_INVALID;
    if (!m->prepared) return mg_fail(m, VOLYM_E_STATE, "volym_mgpu_run: call volym_mgpu_prepare first");
    uint32_t replays = 0;
    double enqueue_us = 0.0;
    const auto t_begin = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); };
    uint32_t done = 0;
    // ---- static view: replay one cycle of the rotating buffers from a captured graph.  One local rank (the deployment: a process
    // per GPU), or several on ONE device over the COPY transport (virtual ranks: every stream is forked from the first rank's march
    // stream and joined back into it, so one hipGraphLaunch carries the frames of all of them) ----
    bool one_device = true;
    for (const MgLocal& L : m->loc) one_device = one_device && L.device == m->loc[0].device;
    const bool graphable = m->loc.size() == 1 || (m->transport == VOLYM_MGPU_COPY && one_device && !m->multi_process);
    if (use_graph && graphable && frames >= 2u * MG_NBUF) {
        MgLocal& L0 = m->loc[0];
        MG_HIP(m, hipSetDevice(L0.device));
        hipStream_t s0 = L0.ctx->slot0().stream;
        const uint64_t view = L0.ctx->slot0().view_serial.load(std::memory_order_relaxed);
        std::vector<hipStream_t> others;                 // every stream but the origin
        for (MgLocal& L : m->loc) { if (&L != &L0) others.push_back(L.ctx->slot0().stream); if (m->world > 1) others.push_back(L.s_comm); }
        if (!m->graph_exec || m->graph_view != view) {
            if (m->graph_exec) { (void)hipGraphExecDestroy(m->graph_exec); m->graph_exec = nullptr; }
            if (m->graph) { (void)hipGraphDestroy(m->graph); m->graph = nullptr; }
            // the work lists must be final (a capture cannot hold the feedback's copies): warm frames, then settle, twice (a
            // measuring list first, then the final one)
            for (int round = 0; round < 2; ++round) {
                for (int w = 0; w < MG_NBUF; ++w) { int rc = mg_enqueue_frame(m, m->frame_no++, false, false); if (rc != VOLYM_OK) return rc; }
                done += MG_NBUF;
                int rc = mg_drain(m);
                if (rc != VOLYM_OK) return rc;
                for (MgLocal& L : m->loc) MG_CTX(m, L, volym_settle(L.ctx));
                if (m->loc.size() == 1) break;
            }
            std::vector<bool> frozen_before;
            for (MgLocal& L : m->loc) { frozen_before.push_back(L.ctx->feedback_frozen); L.ctx->feedback_frozen = true; }
            if (!m->ev_fork && hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming) != hipSuccess) m->ev_fork = nullptr;
            while (m->ev_join.size() < others.size()) {
                hipEvent_t e = nullptr;
                if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) e = nullptr;
                m->ev_join.push_back(e);
            }
            bool ok = m->ev_fork != nullptr;
            for (size_t k = 0; k < others.size(); ++k) ok = ok && m->ev_join[k] != nullptr;
            hipError_t e = ok ? hipStreamBeginCapture(s0, hipStreamCaptureModeThreadLocal) : hipErrorUnknown;
            ok = ok && e == hipSuccess;
            if (ok) {
                // fork: the other streams enter the capture by waiting for a mark of the origin
                if (!others.empty()) {
                    ok = hipEventRecord(m->ev_fork, s0) == hipSuccess;
                    for (size_t k = 0; k < others.size() && ok; ++k) ok = hipStreamWaitEvent(others[k], m->ev_fork, 0) == hipSuccess;
                }
                for (int f = 0; f < MG_NBUF && ok; ++f) ok = mg_enqueue_frame(m, static_cast<uint64_t>(f), true, true) == VOLYM_OK;
                // join: every other stream back into the origin
                for (size_t k = 0; k < others.size() && ok; ++k)
                    ok = hipEventRecord(m->ev_join[k], others[k]) == hipSuccess && hipStreamWaitEvent(s0, m->ev_join[k], 0) == hipSuccess;
                hipGraph_t g = nullptr;
                e = hipStreamEndCapture(s0, &g);
                ok = ok && e == hipSuccess && g != nullptr;
                if (ok) { m->graph = g; ok = hipGraphInstantiate(&m->graph_exec, g, nullptr, nullptr, 0) == hipSuccess; }
                else if (g) (void)hipGraphDestroy(g);
            }
            (void)hipGetLastError();
            for (size_t k = 0; k < m->loc.size(); ++k) {
                m->loc[k].ctx->feedback_frozen = frozen_before[k];
                for (int b = 0; b < MG_NBUF; ++b) m->loc[k].free_pending[b] = false;     // replays start with every buffer free
            }
            if (ok) m->graph_view = view;
            else { if (m->graph_exec) { (void)hipGraphExecDestroy(m->graph_exec); m->graph_exec = nullptr; } m->err.clear(); }
        }
        if (m->graph_exec) {
            std::vector<bool> frozen_before;
            for (MgLocal& L : m->loc) { frozen_before.push_back(L.ctx->feedback_frozen); L.ctx->feedback_frozen = true; }
            const auto t0 = std::chrono::steady_clock::now();
            while (frames - done >= static_cast<uint32_t>(MG_NBUF)) {
                MG_HIP(m, hipGraphLaunch(m->graph_exec, s0));
                done += MG_NBUF;
                replays++;
            }
            // frames enqueued after the replays run on streams that have not seen them: order them behind the origin
            if (!others.empty() && replays) {
                MG_HIP(m, hipEventRecord(m->ev_fork, s0));
                for (hipStream_t x : others) MG_HIP(m, hipStreamWaitEvent(x, m->ev_fork, 0));
            }
            enqueue_us += since(t0);
            // the graph used buffers 0..NBUF-1 in order and ends joined: keep the eager frame counter aligned
            m->frame_no = (m->frame_no + MG_NBUF - 1) / MG_NBUF * MG_NBUF;
            for (size_t k = 0; k < m->loc.size(); ++k) m->loc[k].ctx->feedback_frozen = frozen_before[k];
        }
    }
    {
        const auto t0 = std::chrono::steady_clock::now();
        for (; done < frames; ++done) {
            int rc = mg_enqueue_frame(m, m->frame_no++, false, false);
            if (rc != VOLYM_OK) return rc;
        }
        enqueue_us += since(t0);
    }
    int rc = mg_drain(m);
    if (rc != VOLYM_OK) return rc;
    // a shard that found no slot for a tile stored transparent black in its place: the frames are wrong, say so
    uint32_t over_all = 0;
    for (MgLocal& L : m->loc) {
        uint32_t used = 0, over = 0;
        if (m->world > 1) MG_CTX(m, L, volym_packed_tiles(L.ctx, &used, &over));
        over_all |= over;
    }
    if (timing) {
        timing->wall_ms = since(t_begin) / 1000.0;
        timing->enqueue_us_per_frame = enqueue_us / frames / std::max<size_t>(1, m->loc.size());
        timing->frames = frames;
        timing->graph_replays = replays;
        timing->msg_bytes = static_cast<uint32_t>(m->msg_bytes);
        timing->overflowed = over_all;
    }
    if (over_all) return mg_fail(m, VOLYM_E_STATE, "volym_mgpu_run: a packed shard overflowed the slots volym_mgpu_prepare sized (the view needs more tiles than the probe frame did): call volym_mgpu_prepare again");
    return VOLYM_OK;
}

int volym_mgpu_profile(volym_mgpu* m, uint32_t frames, volym_mgpu_split* split)
{
    if (!m || !split || frames == 0) return VOLYM_E_INVALID;
    if (!m->prepared) return mg_fail(m, VOLYM_E_STATE, "volym_mgpu_profile: call volym_mgpu_prepare first");
    int rc = mg_drain(m);
    if (rc != VOLYM_OK) return rc;
    double march = 0, pack = 0, coll = 0, asem = 0;
    const size_t msg = m->msg_bytes;
    for (uint32_t f = 0; f < frames; ++f) {
        float l_march = 0, l_pack = 0;
        for (MgLocal& L : m->loc) {
            MG_HIP(m, hipSetDevice(L.device));
            hipEvent_t e[3];
            for (auto& x : e) MG_HIP(m, hipEventCreate(&x));
            MG_HIP(m, hipEventRecord(e[0], L.ctx->slot0().stream));
            MG_CTX(m, L, ctx_launch_march(L.ctx));
            MG_HIP(m, hipEventRecord(e[1], L.ctx->slot0().stream));
            if (m->world > 1) MG_CTX(m, L, volym_pack_shard(L.ctx, L.packed[0], msg));
            MG_HIP(m, hipEventRecord(e[2], L.ctx->slot0().stream));
            MG_HIP(m, hipStreamSynchronize(L.ctx->slot0().stream));
            float a = 0, b2 = 0;
            (void)hipEventElapsedTime(&a, e[0], e[1]);
            (void)hipEventElapsedTime(&b2, e[1], e[2]);
            l_march = std::max(l_march, a); l_pack = std::max(l_pack, b2);
            for (auto& x : e) (void)hipEventDestroy(x);
        }
        march += l_march; pack += l_pack;
        // the collective alone (every rank's shard is packed), then the assemble alone
        const auto t0 = std::chrono::steady_clock::now();
        MgLocal* R = m->root >= 0 ? &m->loc[m->root] : nullptr;
        if (m->world > 1) {
            if (m->transport == VOLYM_MGPU_RCCL) {
                MG_NCCL(m, g_rccl.GroupStart());
                ncclResult_t gr = ncclSuccess;
                for (MgLocal& L : m->loc) if (L.rank != 0 && gr == ncclSuccess) gr = g_rccl.Send(L.packed[0], msg, ncclUint8, 0, L.comm, L.s_comm);
                if (R) for (int r = 1; r < m->world && gr == ncclSuccess; ++r) gr = g_rccl.Recv(m->gathered[0] + static_cast<size_t>(r) * msg, msg, ncclUint8, r, R->comm, R->s_comm);
                const ncclResult_t ge = g_rccl.GroupEnd();
                MG_NCCL(m, gr);
                MG_NCCL(m, ge);
            } else {
                MG_HIP(m, hipSetDevice(R->device));
                for (MgLocal& L : m->loc) if (L.rank != 0) MG_HIP(m, hipMemcpyAsync(m->gathered[0] + static_cast<size_t>(L.rank) * msg, L.packed[0], msg, hipMemcpyDefault, R->s_comm));
            }
            for (MgLocal& L : m->loc) { MG_HIP(m, hipSetDevice(L.device)); MG_HIP(m, hipStreamSynchronize(L.s_comm)); }
        }
        coll += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (R && m->world > 1) {
            MG_HIP(m, hipSetDevice(R->device));
            hipEvent_t e0, e1;
            MG_HIP(m, hipEventCreate(&e0)); MG_HIP(m, hipEventCreate(&e1));
            volym_ctx* c = R->ctx;
            MG_HIP(m, hipEventRecord(e0, R->s_comm));
            hipLaunchKernelGGL(volym_assemble_packed_kernel, dim3(c->n_tiles), dim3(256), 0, R->s_comm, m->gathered[0], msg, c->frame_buf(c->slot0()), c->W, c->H,
                               c->tiles_x, c->n_tiles, c->world, c->shard_tiles);
            MG_HIP(m, hipEventRecord(e1, R->s_comm));
            MG_HIP(m, hipStreamSynchronize(R->s_comm));
            float a = 0;
            (void)hipEventElapsedTime(&a, e0, e1);
            asem += a;
            (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        }
    }
    split->march_ms = static_cast<float>(march / frames);
    split->pack_ms = static_cast<float>(pack / frames);
    split->collective_ms = static_cast<float>(coll / frames);
    split->assemble_ms = static_cast<float>(asem / frames);
    return VOLYM_OK;
}

int volym_mgpu_read_rgba8(volym_mgpu* m, uint8_t* out)
{
    if (!m || !out) return VOLYM_E_INVALID;
    if (m->root < 0) return mg_fail(m, VOLYM_E_STATE, "volym_mgpu_read_rgba8: this process does not hold the root rank");
    int rc = mg_drain(m);
    if (rc != VOLYM_OK) return rc;
    MgLocal& R = m->loc[m->root];
    MG_HIP(m, hipSetDevice(R.device));
    MG_HIP(m, hipMemcpy(out, R.ctx->frame_buf(R.ctx->slot0()), static_cast<size_t>(m->W) * m->H * 4, hipMemcpyDeviceToHost));
    return VOLYM_OK;
}

}  // extern "C"
