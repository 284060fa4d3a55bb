// libvolym_hip.so: what the passes over a request's box share beyond the headers (context.hpp declares it).  No C ABI of its own:
// the scan that turns the surface pass's faces per row and the components pass's roots per row into offsets, and the read-back of a
// box-linear volume behind volym_read_component_ids / volym_component_of and volym_read_distance_map / volym_distance_at.
#include <hip/hip_runtime.h>

#include <string>

#include "context.hpp"

using namespace volym;

static int fail(volym_ctx* c, int code, const std::string& msg) { return ctx_fail(c, code, msg); }
#define HIPCHK(ctx, expr) VOLYM_HIPCHK(ctx, expr)

namespace volym {

// ---- the scan of the row counts: three plain phases, no workgroup waits for another --------------------------------------------
// rows[] in blocks of SCAN_ROWS = 256: (1) the sum of every block, (2) one workgroup turns the block sums into their exclusive
// prefix, in place, (3) every block scans its own rows, in place, from its prefix.  Sums wrap at 2^32; a pass whose total can reach
// that refuses it before any offset is used.
constexpr uint32_t SCAN_ROWS = 256u;                               // one row per thread of a 256-thread workgroup
static_assert(SCAN_ROWS == VOLYM_SURFACE_SCAN_ROWS, "RowOffsets sizes the block sums by the public constant");

// exclusive prefix of v over the 256 threads of the workgroup; *sum (if not NULL) the total
__device__ __forceinline__ uint32_t box_block_scan(uint32_t v, uint32_t* s_scan, uint32_t* sum)
{
    const uint32_t t = threadIdx.x;
    s_scan[t] = v;
    __syncthreads();
    for (uint32_t step = 1u; step < 256u; step <<= 1) {
        const uint32_t add = t >= step ? s_scan[t - step] : 0u;
        __syncthreads();
        s_scan[t] += add;
        __syncthreads();
    }
    const uint32_t inclusive = s_scan[t];
    if (sum) *sum = s_scan[255];
    __syncthreads();                                               // (s_scan may be used again)
    return inclusive - v;
}

__global__ __launch_bounds__(256) void volym_box_scan_sums_kernel(const uint32_t* __restrict__ rows, uint32_t* __restrict__ sums, uint32_t n_rows)
{
    __shared__ uint32_t s_scan[256];
    const uint32_t i = blockIdx.x * SCAN_ROWS + threadIdx.x;
    uint32_t sum;
    (void)box_block_scan(i < n_rows ? rows[i] : 0u, s_scan, &sum);
    if (threadIdx.x == 0u) sums[blockIdx.x] = sum;
}

// one workgroup; thread t owns the ceil(n_blocks / 256) consecutive sums from t * per on
__global__ __launch_bounds__(256) void volym_box_scan_blocks_kernel(uint32_t* __restrict__ sums, uint32_t n_blocks)
{
    __shared__ uint32_t s_scan[256];
    const uint32_t per = (n_blocks + 255u) / 256u;
    const uint32_t b0 = min(threadIdx.x * per, n_blocks), b1 = min(b0 + per, n_blocks);
    uint32_t mine = 0u;
    for (uint32_t b = b0; b < b1; ++b) mine += sums[b];
    uint32_t run = box_block_scan(mine, s_scan, nullptr);
    for (uint32_t b = b0; b < b1; ++b) { const uint32_t v = sums[b]; sums[b] = run; run += v; }
}

__global__ __launch_bounds__(256) void volym_box_scan_rows_kernel(uint32_t* __restrict__ rows, const uint32_t* __restrict__ sums, uint32_t n_rows)
{
    __shared__ uint32_t s_scan[256];
    const uint32_t i = blockIdx.x * SCAN_ROWS + threadIdx.x;
    const uint32_t before = box_block_scan(i < n_rows ? rows[i] : 0u, s_scan, nullptr);
    if (i < n_rows) rows[i] = sums[blockIdx.x] + before;
}

// (n_rows > 0; a grid of one workgroup runs the same three phases)
int scan_row_offsets(volym_ctx* c, hipStream_t stream, const RowOffsets& offsets, uint32_t n_rows)
{
    uint32_t* const rows = offsets.rows.ptr;
    uint32_t* const sums = offsets.sums.ptr;
    const uint32_t n_blocks = (n_rows + SCAN_ROWS - 1u) / SCAN_ROWS;
    hipLaunchKernelGGL(volym_box_scan_sums_kernel, dim3(n_blocks), dim3(256), 0, stream, rows, sums, n_rows);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(volym_box_scan_blocks_kernel, dim3(1), dim3(256), 0, stream, sums, n_blocks);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(volym_box_scan_rows_kernel, dim3(n_blocks), dim3(256), 0, stream, rows, sums, n_rows);
    HIPCHK(c, hipGetLastError());
    return VOLYM_OK;
}

// ---- a box-linear uint32 volume back to the host -------------------------------------------------------------------------------
static const uint32_t* box_word(const uint32_t box[6], const uint32_t* src, uint32_t x, uint32_t y, uint32_t z)
{
    const size_t w = box[3] - box[0], h = box[4] - box[1];
    return src + (x - box[0]) + w * ((y - box[1]) + h * static_cast<size_t>(z - box[2]));
}

int read_box_volume(volym_ctx* c, const char* who, const char* pass, bool have, const uint32_t box[6], const uint32_t* src, const uint32_t sub[6],
                    uint32_t* out)
{
    const std::string name(who);
    if (!have) return fail(c, VOLYM_E_STATE, name + ": no " + pass + " since the volume was set");
    if (!sub) sub = box;
    for (int k = 0; k < 3; ++k)
        if (sub[k] > sub[3 + k] || sub[k] < box[k] || sub[3 + k] > box[3 + k])
            return fail(c, VOLYM_E_INVALID, name + ": the sub-box must have lo <= hi and lie inside the box of the pass");
    if (box_texels(sub) == 0u) return VOLYM_OK;
    if (!out) return fail(c, VOLYM_E_INVALID, name + ": NULL output");
    HIPCHK(c, hipSetDevice(c->device));
    const hipStream_t stream = c->slot0().stream;
    const size_t w = box[3] - box[0], h = box[4] - box[1];
    const size_t sw = sub[3] - sub[0], sh = sub[4] - sub[1], sd = sub[5] - sub[2];
    src = box_word(box, src, sub[0], sub[1], sub[2]);
    if (sw == w && sh == h) {
        HIPCHK(c, hipMemcpyAsync(out, src, sw * sh * sd * 4u, hipMemcpyDeviceToHost, stream));        // whole slices: one run
    } else {
        for (size_t z = 0; z < sd; ++z)                 // one pitched copy per slice of the sub-box
            HIPCHK(c, hipMemcpy2DAsync(out + z * sw * sh, sw * 4u, src + z * w * h, w * 4u, sw * 4u, sh, hipMemcpyDeviceToHost, stream));
    }
    HIPCHK(c, hipStreamSynchronize(stream));
    return VOLYM_OK;
}

int read_box_texel(volym_ctx* c, const char* who, const char* pass, bool have, const uint32_t box[6], const uint32_t* src, uint32_t x, uint32_t y,
                   uint32_t z, uint32_t* out)
{
    const std::string name(who);
    if (!out) return fail(c, VOLYM_E_INVALID, name + ": NULL output");
    if (!have) return fail(c, VOLYM_E_STATE, name + ": no " + pass + " since the volume was set");
    if (x < box[0] || x >= box[3] || y < box[1] || y >= box[4] || z < box[2] || z >= box[5])
        return fail(c, VOLYM_E_INVALID, name + ": the texel lies outside the box of the pass");
    return read_back(c, c->slot0().stream, out, box_word(box, src, x, y, z), sizeof *out);
}

}  // namespace volym
