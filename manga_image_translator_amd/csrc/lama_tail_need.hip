// lama_tail_need.hip — which parts of LaMa's decoder tail the composite reads: the live-cell map of the 7x7 output convolution and the
// live-block lists of the three stride-2 transposed convolutions (MitConvGemm.live_blocks), from the page masks, on the caller's stream.
//
// lama_post_kernel takes the network's prediction only where mask >= 127 (keep_inpainted).  Everything behind the FFC blocks is local, so
// the need propagates backwards as byte maps (manga_image_translator_amd/lama.py tail_need_numpy states the same in numpy):
//   need_pred = mask >= 127                                     [H, W]
//   need_u3   = dilate(need_pred, 3)                            the 7x7 window (reflection stays inside it)
//   S2        = pool2x2_any(need_u3)                            ups[2]'s parity sub-grid [H/2, W/2]: OR over the 2 x 2 output parities
//   S1        = pool2x2_any(dilate(S2, 1))                      ups[1]'s sub-grid [H/4, W/4]; input i feeds outputs 2i-1, 2i, 2i+1, so
//   S0        = pool2x2_any(dilate(S1, 1))                      dilate(pool) is a superset of the inputs a needed output reads
// A sub-grid block of 8 x 8 positions is live when it holds a set byte.  The lists are written in block-raster order, image after
// image (a flag per block, a count per image, then a scan: no arrival-order append), so a step's launches do not depend on timing.
// Nothing in the reference corresponds to it (the reference computes the whole page).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mit_hip.h"
#include "common.h"

namespace {

// T[b][y][j] = any need_pred[b][y][2j-3 .. 2j+4]   (the 7-wide window of both pixels of the column pair)
__global__ __launch_bounds__(256) void need_rows_kernel(const uint8_t *__restrict__ mask, uint8_t *__restrict__ T, const int W, const int w2, const int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int j = (int)(idx % w2);
    const uint8_t *row = mask + (idx / w2) * W;
    const int x0 = 2 * j - 3 < 0 ? 0 : 2 * j - 3, x1 = 2 * j + 4 >= W ? W - 1 : 2 * j + 4;
    bool any = false;
    for (int x = x0; x <= x1; ++x) any = any || row[x] >= 127;
    T[idx] = any;
}

// dst[b][i][j] = any src[b][2i-R .. 2i+1+R][2j-RX .. 2j+1+RX]: pool2x2_any of a dilation by R rows and RX columns.  POOLX = false: the
// columns were pooled before (need_rows_kernel), column j reads column j
template <int R, int RX, bool POOLX>
__global__ __launch_bounds__(256) void need_pool_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const int hs, const int ws, const int hd,
                                                        const int wd, const int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int j = (int)(idx % wd), i = (int)((idx / wd) % hd);
    const uint8_t *img = src + (idx / ((int64_t)wd * hd)) * hs * ws;
    const int y0 = 2 * i - R < 0 ? 0 : 2 * i - R, y1 = 2 * i + 1 + R >= hs ? hs - 1 : 2 * i + 1 + R;
    const int x0 = !POOLX ? j : (2 * j - RX < 0 ? 0 : 2 * j - RX), x1 = !POOLX ? j : (2 * j + 1 + RX >= ws ? ws - 1 : 2 * j + 1 + RX);
    bool any = false;
    for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x) any = any || img[(int64_t)y * ws + x] != 0;
    dst[idx] = any;
}

// cells[b][cy][cx] = any need_pred in the 8-row x 32-column cell
__global__ __launch_bounds__(256) void need_cells_kernel(const uint8_t *__restrict__ mask, uint8_t *__restrict__ cells, const int H, const int W, const int ch,
                                                         const int cw, const int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int cx = (int)(idx % cw), cy = (int)((idx / cw) % ch);
    const uint8_t *img = mask + (idx / ((int64_t)cw * ch)) * H * W;
    const int y1 = cy * 8 + 8 > H ? H : cy * 8 + 8, x1 = cx * 32 + 32 > W ? W : cx * 32 + 32;
    bool any = false;
    for (int y = cy * 8; y < y1; ++y)
        for (int x = cx * 32; x < x1; ++x) any = any || img[(int64_t)y * W + x] >= 127;
    cells[idx] = any;
}

struct NeedLevels {
    const uint8_t *S[3];  // sub-grid need maps [B][h][w]
    uint8_t *flag[3];     // [B][blocks per image]: the block holds a set byte
    int h[3], w[3];
    int32_t *list[3], *start[3], *count[3];
};

// flag[level][b][t] = block t of image b holds a set byte: one thread per block.  grid (ceil(B * bpi_max / 256), 3)
__global__ __launch_bounds__(256) void need_flags_kernel(const NeedLevels lv, const int B) {
    const int l = blockIdx.y, h = lv.h[l], w = lv.w[l];
    const int bw = (w + 7) >> 3, bpi = ((h + 7) >> 3) * bw;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= B * bpi) return;
    const int b = idx / bpi, t = idx - b * bpi;
    const int by = t / bw, bx = t - by * bw;
    const uint8_t *img = lv.S[l] + (int64_t)b * h * w;
    const int y1 = by * 8 + 8 > h ? h : by * 8 + 8, x1 = bx * 8 + 8 > w ? w : bx * 8 + 8;
    bool any = false;
    for (int y = by * 8; y < y1; ++y)
        for (int x = bx * 8; x < x1; ++x) any = any || img[y * w + x] != 0;
    lv.flag[l][idx] = any;
}

// count[level][b] = live blocks of image b.  grid (B, 3)
__global__ __launch_bounds__(256) void need_count_kernel(const NeedLevels lv) {
    const int l = blockIdx.y, b = blockIdx.x;
    const int bpi = ((lv.h[l] + 7) >> 3) * ((lv.w[l] + 7) >> 3);
    const uint8_t *flag = lv.flag[l] + (int64_t)b * bpi;
    int n = 0;
    for (int t = threadIdx.x; t < bpi; t += 256) n += flag[t];
    __shared__ int wsum[4];
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) lv.count[l][b] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// start[level][b] = live blocks of the images before b (start[B] = all); list[start[b] ..] = ids b * bpi + t of b's live blocks, t ascending
__global__ __launch_bounds__(256) void need_fill_kernel(const NeedLevels lv, const int B) {
    const int l = blockIdx.y, b = blockIdx.x;
    const int bpi = ((lv.h[l] + 7) >> 3) * ((lv.w[l] + 7) >> 3);
    const uint8_t *flag = lv.flag[l] + (int64_t)b * bpi;
    int base = 0;
    for (int i = 0; i < b; ++i) base += lv.count[l][i];
    if (threadIdx.x == 0) {
        lv.start[l][b] = base;
        if (b == B - 1) lv.start[l][B] = base + lv.count[l][b];
    }
    __shared__ int wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t *out = lv.list[l];
    for (int t0 = 0; t0 < bpi; t0 += 256) {
        const int t = t0 + threadIdx.x;
        const bool live = t < bpi && flag[t] != 0;
        const unsigned long long bal = __ballot(live);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        __syncthreads();  // the previous chunk's sums have been read
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int pos = base + before;
        for (int i = 0; i < wave; ++i) pos += wsum[i];
        if (live) out[pos] = b * bpi + t;
        base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    }
}

struct Sizes {
    int64_t T, S[3], F[3], counts, total;
};
Sizes sizes_of(int B, int H, int W) {
    Sizes z;
    z.counts = ((int64_t)3 * B * 4 + 15) / 16 * 16;
    z.T = ((int64_t)B * H * (W / 2) + 15) / 16 * 16;
    z.total = z.counts + z.T;
    for (int l = 0; l < 3; ++l) {
        const int h = H >> (3 - l), w = W >> (3 - l);
        z.S[l] = ((int64_t)B * h * w + 15) / 16 * 16;
        z.F[l] = ((int64_t)B * ((h + 7) / 8) * ((w + 7) / 8) + 15) / 16 * 16;
        z.total += z.S[l] + z.F[l];
    }
    return z;
}

}  // namespace

extern "C" int64_t mit_lama_tail_need_work(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return sizes_of(B, H, W).total;
}

extern "C" int mit_lama_tail_need(const uint8_t *mask_dev, int B, int H, int W, uint8_t *cells_dev, int32_t *list0_dev, int32_t *start0_dev,
                                  int32_t *list1_dev, int32_t *start1_dev, int32_t *list2_dev, int32_t *start2_dev, uint8_t *work_dev, void *stream) {
    if (!mask_dev || !cells_dev || !list0_dev || !start0_dev || !list1_dev || !start1_dev || !list2_dev || !start2_dev || !work_dev)
        return mit_set_error("mit_lama_tail_need: null pointer");
    if (B <= 0 || B > 65535 || H <= 0 || W <= 0 || (H & 7) || (W & 7)) return mit_set_error("mit_lama_tail_need: need 0 < B < 65536 and H, W multiples of 8 (got %d x %d x %d)", B, H, W);
    if ((int64_t)B * H * W > 0x7fffffffLL) return mit_set_error("mit_lama_tail_need: B * H * W must stay below 2^31");
    if (reinterpret_cast<uintptr_t>(work_dev) & 15) return mit_set_error("mit_lama_tail_need: work must be 16-byte aligned");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const Sizes z = sizes_of(B, H, W);
    int32_t *counts = reinterpret_cast<int32_t *>(work_dev);
    uint8_t *T = work_dev + z.counts;
    uint8_t *S0 = T + z.T, *S1 = S0 + z.S[0], *S2 = S1 + z.S[1];
    uint8_t *F0 = S2 + z.S[2], *F1 = F0 + z.F[0], *F2 = F1 + z.F[1];
    auto blocks = [](int64_t n) { return dim3((unsigned)((n + 255) / 256)); };
    const int ch = H / 8, cw = (W + 31) / 32;
    int64_t n = (int64_t)B * ch * cw;
    hipLaunchKernelGGL(need_cells_kernel, blocks(n), dim3(256), 0, s, mask_dev, cells_dev, H, W, ch, cw, n);
    n = (int64_t)B * H * (W / 2);
    hipLaunchKernelGGL(need_rows_kernel, blocks(n), dim3(256), 0, s, mask_dev, T, W, W / 2, n);
    n = (int64_t)B * (H / 2) * (W / 2);
    hipLaunchKernelGGL((need_pool_kernel<3, 0, false>), blocks(n), dim3(256), 0, s, T, S2, H, W / 2, H / 2, W / 2, n);  // rows 2i-3 .. 2i+4 of T: one column
    n = (int64_t)B * (H / 4) * (W / 4);
    hipLaunchKernelGGL((need_pool_kernel<1, 1, true>), blocks(n), dim3(256), 0, s, S2, S1, H / 2, W / 2, H / 4, W / 4, n);
    n = (int64_t)B * (H / 8) * (W / 8);
    hipLaunchKernelGGL((need_pool_kernel<1, 1, true>), blocks(n), dim3(256), 0, s, S1, S0, H / 4, W / 4, H / 8, W / 8, n);
    NeedLevels lv;
    const uint8_t *Sl[3] = {S0, S1, S2};
    uint8_t *Fl[3] = {F0, F1, F2};
    int32_t *lists[3] = {list0_dev, list1_dev, list2_dev}, *starts[3] = {start0_dev, start1_dev, start2_dev};
    for (int l = 0; l < 3; ++l) {
        lv.S[l] = Sl[l], lv.flag[l] = Fl[l], lv.h[l] = H >> (3 - l), lv.w[l] = W >> (3 - l);
        lv.list[l] = lists[l], lv.start[l] = starts[l], lv.count[l] = counts + l * B;
    }
    hipLaunchKernelGGL(need_flags_kernel, dim3((unsigned)((z.F[2] + 255) / 256), 3), dim3(256), 0, s, lv, B);  // (level 2 has the most blocks)
    hipLaunchKernelGGL(need_count_kernel, dim3(B, 3), dim3(256), 0, s, lv);
    hipLaunchKernelGGL(need_fill_kernel, dim3(B, 3), dim3(256), 0, s, lv, B);
    MIT_CHECK_LAUNCH("mit_lama_tail_need");
    return 0;
}
