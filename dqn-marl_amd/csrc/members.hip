// Member blocks of [members][...] arrays copied from donor to receiver, every array and every
// receiver in one launch (evx_copy_members in include/evacx.h; evacx.population.copy_members: the
// exploit step of population-based training).
//
// A population keeps every per-member buffer -- flat parameters, target parameters, Adam moments,
// the MFMA operand copies of both nets -- as one slice of a [members][...] array, so "member dst
// takes member src's weights" is, per array, a copy of one block onto another at a fixed stride.
// The grid is (chunk, receiver, buffer): blockIdx.z picks the array, blockIdx.y the receiver (the
// members with src[k] != k, listed compactly by the host), blockIdx.x strides over the block.
// The buffer table and the receiver list reach the kernel by value (1280 bytes of kernel
// arguments; they are wave-uniform, so reading them costs scalar loads only).
//
// Two copy paths, chosen per (receiver, buffer), wave-uniform:
//   * the receiver's and the donor's block are congruent mod 16: up to three 4-byte words bring
//     both to a 16-byte boundary, then 16 bytes per lane (a wave-instruction moves 1 KiB,
//     coalesced), then up to three 4-byte words of tail;
//   * otherwise 4 bytes per lane (256 contiguous bytes per wave-instruction): no 16-byte access can
//     be aligned on both sides. A member's flat parameters are 504 837 floats, a stride of 4 mod 16,
//     so this is the path of every flat buffer unless dst - src is a multiple of 4.
// Plain vector loads and stores: no LDS, no atomics, nothing shared between workgroups. The donor
// blocks are never written in the launch (the host refuses a donor that is itself replaced), so
// no block reads what another writes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "evacx.h"
#include "evx_host.h"

namespace evxc {
constexpr int NT = 256;
constexpr int MAX_MEMBERS = 64, MAX_BUFS = 32;
// bytes one workgroup moves per pass of the 16-byte path: the unit the chunk count is sized by
constexpr int64_t PASS_BYTES = (int64_t)NT * 16;
// workgroups of one launch the chunk count aims at: 256 CUs x 8 resident workgroups x 4. Most
// (receiver, buffer) pairs of a population are small (biases, the fc3 operands) and their
// workgroups leave at once, so the large blocks still spread over every CU.
constexpr int64_t GRID_TARGET = 8192;

using evxh::fail;
using evxh::failf;

struct CopyArgs {
    evx_member_buf buf[MAX_BUFS];
    int32_t dst[MAX_MEMBERS];
    int32_t src[MAX_MEMBERS];
};

__global__ __launch_bounds__(NT) void copy_members_kernel(CopyArgs a) {
    const evx_member_buf b = a.buf[blockIdx.z];
    const int d = a.dst[blockIdx.y], s = a.src[blockIdx.y];
    char* __restrict__ D = (char*)b.base + (int64_t)d * b.stride_bytes;
    const char* __restrict__ S = (const char*)b.base + (int64_t)s * b.stride_bytes;
    const int64_t n = b.bytes;
    const int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x, nt = (int64_t)gridDim.x * NT;
    if ((((uintptr_t)D ^ (uintptr_t)S) & 15) == 0) {
        int64_t head = (int64_t)((0 - (uintptr_t)D) & 15);  // 0, 4, 8 or 12 bytes to the boundary
        if (head > n) head = n;
        const int64_t n16 = (n - head) >> 4;
        const int64_t tail0 = head + (n16 << 4);  // [tail0, n): 0..3 words
        const uint4* __restrict__ S16 = (const uint4*)(S + head);
        uint4* __restrict__ D16 = (uint4*)(D + head);
#pragma unroll 4
        for (int64_t i = t; i < n16; i += nt) D16[i] = S16[i];
        if (blockIdx.x == 0) {  // lanes 0..2: the head's words, lanes 4..6: the tail's
            const int lane = threadIdx.x;
            if (lane < 3 && 4 * (int64_t)lane < head) ((uint32_t*)D)[lane] = ((const uint32_t*)S)[lane];
            const int64_t o = tail0 + 4 * (int64_t)(lane - 4);
            if (lane >= 4 && lane < 7 && o < n) *(uint32_t*)(D + o) = *(const uint32_t*)(S + o);
        }
    } else {
        const int64_t n4 = n >> 2;
        const uint32_t* __restrict__ S4 = (const uint32_t*)S;
        uint32_t* __restrict__ D4 = (uint32_t*)D;
#pragma unroll 4
        for (int64_t i = t; i < n4; i += nt) D4[i] = S4[i];
    }
}
}  // namespace evxc

extern "C" {

int evx_copy_members(const evx_member_buf* bufs, int32_t nbufs, const int32_t* src, int32_t members, void* stream) {
    using namespace evxc;
    if (!bufs || !src) return fail(-22, "copy_members: NULL argument");
    if (members < 1 || members > MAX_MEMBERS)
        return failf(-22, "copy_members: members must be 1..%d, not %d", MAX_MEMBERS, members);
    if (nbufs < 1 || nbufs > MAX_BUFS) return failf(-22, "copy_members: nbufs must be 1..%d, not %d", MAX_BUFS, nbufs);
    for (int k = 0; k < members; k++)
        if (src[k] < 0 || src[k] >= members)
            return failf(-22, "copy_members: src[%d] = %d is outside 0..%d", k, src[k], members - 1);
    for (int k = 0; k < members; k++)
        if (src[src[k]] != src[k])
            return failf(-22, "copy_members: member %d takes from member %d, which is itself replaced (by %d)", k,
                         src[k], src[src[k]]);
    CopyArgs a{};
    int64_t longest = 0;
    for (int i = 0; i < nbufs; i++) {
        const evx_member_buf& b = bufs[i];
        if (!b.base) return failf(-22, "copy_members: buffer %d has a NULL base", i);
        if (((uintptr_t)b.base & 3) || (b.stride_bytes & 3) || (b.bytes & 3))
            return failf(-22,
                         "copy_members: buffer %d: base, stride_bytes = %lld and bytes = %lld must be multiples of 4", i,
                         (long long)b.stride_bytes, (long long)b.bytes);
        if (b.bytes < 0 || b.bytes > b.stride_bytes)
            return failf(-22, "copy_members: buffer %d: bytes = %lld must lie in 0..stride_bytes = %lld", i,
                         (long long)b.bytes, (long long)b.stride_bytes);
        a.buf[i] = b;
        if (b.bytes > longest) longest = b.bytes;
    }
    int nrecv = 0;
    for (int k = 0; k < members; k++)
        if (src[k] != k) {
            a.dst[nrecv] = k;
            a.src[nrecv++] = src[k];
        }
    if (nrecv == 0 || longest == 0) return 0;  // the identity map, or nothing to move: no launch
    const int64_t pairs = (int64_t)nrecv * nbufs;
    int64_t chunks = (longest + PASS_BYTES - 1) / PASS_BYTES;
    const int64_t cap = GRID_TARGET / pairs > 1 ? GRID_TARGET / pairs : 1;
    if (chunks > cap) chunks = cap;
    hipLaunchKernelGGL(copy_members_kernel, dim3((unsigned)chunks, (unsigned)nrecv, (unsigned)nbufs), dim3(NT), 0,
                       (hipStream_t)stream, a);
    return evxh::hip_status("copy_members launch");
}

}  // extern "C"
