// rotating.hip -- row moves of the rotating KV cache (RotatingKVCache, cache/kv_cache/rotating.py).
//
// The cache keeps the reference's row order in its buffers [Hkv, cap, D]: the first `keep` rows are the sink positions, the rest a
// ring.  Two host-known events rearrange the rows, each one launch pair per layer outside any captured graph:
//   - a full ring before a multi-row update is put into temporal order (the rows after the write slot first);
//   - a store longer than the window (a long prompt, a chunk) is cut to [sinks, newest window - keep] before the next single-row update.
// Both are dst row keep + j <- src row keep + (j + shift) % n for j < n_dst: k_ring_gather copies them into a scratch, k_ring_put back.
#include "common.hpp"

namespace {

template <int D>
__global__ void __launch_bounds__(256) k_ring_gather(const u16 *k, const u16 *v, int H, int cap, int keep, int n, int shift, int n_dst,
                                                     u16 *scratch) {
    constexpr int LPT = D / 8;
    const long long r = (long long)blockIdx.x * (256 / LPT) + threadIdx.x / LPT;  // (head, j)
    if (r >= (long long)H * n_dst) return;
    const int h = (int)(r / n_dst), j = (int)(r % n_dst), dc = threadIdx.x % LPT;
    const size_t src = ((size_t)h * cap + keep + (j + shift) % n) * D + dc * 8;
    const size_t dst = (size_t)r * D + dc * 8, half = (size_t)H * n_dst * D;
    const u16 *base = blockIdx.y ? v : k;
    *reinterpret_cast<uint4 *>(scratch + (blockIdx.y ? half : 0) + dst) = *reinterpret_cast<const uint4 *>(base + src);
}

template <int D>
__global__ void __launch_bounds__(256) k_ring_put(u16 *k, u16 *v, int H, int cap, int keep, int n_dst, const u16 *scratch) {
    constexpr int LPT = D / 8;
    const long long r = (long long)blockIdx.x * (256 / LPT) + threadIdx.x / LPT;
    if (r >= (long long)H * n_dst) return;
    const int h = (int)(r / n_dst), j = (int)(r % n_dst), dc = threadIdx.x % LPT;
    const size_t half = (size_t)H * n_dst * D;
    u16 *base = blockIdx.y ? v : k;
    *reinterpret_cast<uint4 *>(base + ((size_t)h * cap + keep + j) * D + dc * 8) =
        *reinterpret_cast<const uint4 *>(scratch + (blockIdx.y ? half : 0) + (size_t)r * D + dc * 8);
}

template <int D>
void ring_order_d(u16 *k, u16 *v, int H, int cap, int keep, int n, int shift, int n_dst, u16 *scratch, hipStream_t st) {
    const int per_block = 256 / (D / 8);
    const dim3 grid((unsigned)(((long long)H * n_dst + per_block - 1) / per_block), 2);
    hipLaunchKernelGGL(k_ring_gather<D>, grid, dim3(256), 0, st, k, v, H, cap, keep, n, shift, n_dst, scratch);
    hipLaunchKernelGGL(k_ring_put<D>, grid, dim3(256), 0, st, k, v, H, cap, keep, n_dst, scratch);
}

}  // namespace

extern "C" int pie_kv_ring_order(void *k, void *v, int H, int cap, int head_dim, int keep, int n, int shift, int n_dst, void *scratch,
                                 void *stream) {
    PIE_REQUIRE(k && v && scratch, PIE_E_ARG, "pie_kv_ring_order: null pointer");
    PIE_REQUIRE(head_dim == 64 || head_dim == 128, PIE_E_SHAPE, "pie_kv_ring_order: head_dim must be 64 or 128");
    PIE_REQUIRE(H > 0 && keep >= 0 && n >= 1 && n_dst >= 0 && n_dst <= n && shift >= 0 && keep + n <= cap, PIE_E_SHAPE,
                "pie_kv_ring_order: need 0 <= n_dst <= n, keep + n <= cap, shift >= 0");
    PIE_REQUIRE(pie_aligned(k, 16) && pie_aligned(v, 16) && pie_aligned(scratch, 16), PIE_E_ALIGN, "pie_kv_ring_order: misaligned pointer");
    if (n_dst == 0) return PIE_OK;
    hipStream_t st = (hipStream_t)stream;
    if (head_dim == 128) ring_order_d<128>((u16 *)k, (u16 *)v, H, cap, keep, n, shift % n, n_dst, (u16 *)scratch, st);
    else ring_order_d<64>((u16 *)k, (u16 *)v, H, cap, keep, n, shift % n, n_dst, (u16 *)scratch, st);
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}
