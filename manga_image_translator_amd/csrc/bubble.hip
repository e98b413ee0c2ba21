// bubble.hip — the --ignore-bubble rules on the device: the bubble stage of the mask refinement and the OCR models' crop test.
//
// Reference: manga_translator/mask_refinement/__init__.py:31-50 (dilate the refined mask, walk its external contours, erase the ones whose
// page rectangle is_ignore() rejects), utils/bubble.py:28-84 (is_ignore: share of dark values in a 2-pixel frame, then the colour test),
// called per rectified crop from ocr/model_48px_ctc.py:90, ocr/model_32px.py:84 and manga_translator.py:1358.  The host statements are
// mask_refinement.bubble_filter and textline.is_ignore; these kernels give their bytes.
//
// Everything that decides is an integer.  The frame rule `ignore_bubble <= round(v / total, 6) * 100 <= 100 - ignore_bubble` is monotone
// in the count v, so the host hands over the integer interval [lo, hi] of v for which Python's own expression is true
// (mask_refinement.bubble_interval) and the device compares counts.  The colour rule `sum_c (c - gray)^2 > 100`, gray = 0.299 r + 0.587 g
// + 0.114 b in float64, is stated in thousandths: sum_c (1000 c - G)^2 > 10^8 with G = 299 r + 587 g + 114 b in 64-bit integers — equal
// on all 2^24 colours, none of which meets the threshold exactly (tests/test_bubble_rules.py).
//
// mit_bubble_filter, passes over the page (P = H * W, each HBM / atomic bound, a few int32 or byte planes read or written once):
//   1. dilation by a k x k square, anchor k / 2, as a row maximum then a column maximum (taps outside the image do not count);
//   2. RETR_EXTERNAL as hole filling: the background is labelled 4-connected, the labels that reach the page border are outside, every
//      other pixel is filled;
//   3. the filled map is labelled 8-connected (lock-free union-find on the raster index, root = smallest index, as mask_assign.hip and
//      ctd_refine.hip do) and every root collects its bounding rectangle with integer atomics issued by its rim pixels only;
//   4. row prefix sums of `coloured` (0 / 1 per pixel) and of the bright elements of the page's 2-pixel frame (0..3 per pixel); one wave
//      per component then adds, over the rows of its rectangle (one pixel larger to the right and below, clamped), two differences of
//      prefix sums per row.  A component that covers the page costs H row reads; several hundred overlapping rectangles cost their
//      heights, not their areas;
//   5. the pixels of the components judged so are cleared in the dilated mask.
// The tables are sized by P (the root list too): no cap on the number of components.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mit_hip.h"
#include "common.h"

namespace {

constexpr int INT_PLANES = 8;     // L, x0, y0, x1, y1, prefix of coloured, prefix of bright frame elements, root list
constexpr int BYTE_PLANES = 3;    // row maxima, the map being labelled (background, then filled), one flag per root (outside, then erase)
constexpr int STATUS_BYTES = 64;  // status[0]: number of components

struct Planes {
    int *status, *L, *x0, *y0, *x1, *y1, *sc, *sb, *list;
    uint8_t *tmp, *on, *flag;
};

Planes carve(void *ws, int64_t P) {
    int *s = static_cast<int *>(ws);
    int *b = s + STATUS_BYTES / sizeof(int);
    uint8_t *u = reinterpret_cast<uint8_t *>(b + INT_PLANES * P);
    return Planes{s, b, b + P, b + 2 * P, b + 3 * P, b + 4 * P, b + 5 * P, b + 6 * P, b + 7 * P, u, u + P, u + 2 * P};
}

__device__ __forceinline__ int uf_find(const int *__restrict__ L, int a) {
    int r = a;
    for (;;) {
        const int q = __atomic_load_n(&L[r], __ATOMIC_RELAXED);
        if (q == r) return r;
        r = q;
    }
}

__device__ __forceinline__ void uf_union(int *__restrict__ L, int a, int b) {
    for (;;) {
        a = uf_find(L, a);
        b = uf_find(L, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&L[a], b);  // a > b: hang the larger root under the smaller
        if (old == a) return;
        a = old;  // someone re-rooted a meanwhile: retry from there
    }
}

// dst(x) = max over taps t = 0..k-1 of src(x + t - k / 2), taps outside the row ignored (cv2.dilate's default anchor and border).
__global__ __launch_bounds__(256) void row_max_kernel(const uint8_t *__restrict__ src, int W, int64_t P, int k, uint8_t *__restrict__ dst) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int64_t y = p / W;
    const int x = (int)(p - y * W);
    const int a = max(x - k / 2, 0), b = min(x - k / 2 + k - 1, W - 1);
    const uint8_t *row = src + y * W;
    int v = 0;
    for (int i = a; i <= b; ++i) v = max(v, (int)row[i]);
    dst[p] = (uint8_t)v;
}

// the same down the columns; also writes the background map the hole filling labels
__global__ __launch_bounds__(256) void col_max_kernel(const uint8_t *__restrict__ src, int H, int W, int64_t P, int k, uint8_t *__restrict__ dst,
                                                      uint8_t *__restrict__ background) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int y = (int)(p / W);
    const int x = (int)(p - (int64_t)y * W);
    const int a = max(y - k / 2, 0), b = min(y - k / 2 + k - 1, H - 1);
    int v = 0;
    for (int i = a; i <= b; ++i) v = max(v, (int)src[(int64_t)i * W + x]);
    dst[p] = (uint8_t)v;
    background[p] = v == 0;
}

// The 64 pixels of a wave are consecutive in raster order: a horizontal run of set pixels inside it (and inside one row) starts its
// life already linked to its first pixel, so link_kernel only joins runs across wave boundaries and rows.
template <bool BOXES>
__global__ __launch_bounds__(256) void init_kernel(const uint8_t *__restrict__ on, int W, int64_t P, Planes pl) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool ok = p < P;
    const bool t = ok && on[p] != 0;
    const int x = ok ? (int)(p % W) : 0;
    const int lane = threadIdx.x & 63;
    const unsigned long long cm = __ballot(t);
    const bool start = t && (lane == 0 || !((cm >> (lane - 1)) & 1ull) || x == 0);
    const unsigned long long sm = __ballot(start);
    if (!ok) return;
    if (!t) {
        pl.L[p] = -1;
        return;
    }
    pl.L[p] = (int)p - (lane - (63 - __clzll((long long)(sm & ((2ull << lane) - 1ull)))));
    if (BOXES) {
        pl.x0[p] = INT32_MAX;
        pl.y0[p] = INT32_MAX;
        pl.x1[p] = 0;
        pl.y1[p] = 0;
    }
}

// Only the unions that can join two sets: (left) runs are pre-linked inside a wave, so only its first lane looks left; (up) not when
// the left neighbour and the pixel above it are set too — the left neighbour makes that link; (diagonals, 8-connectivity only) only
// when neither the pixel above nor the horizontal neighbour below the diagonal can.
template <bool CONN8>
__global__ __launch_bounds__(256) void link_kernel(const uint8_t *__restrict__ on, int W, int64_t P, int *__restrict__ L) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P || !on[p]) return;
    const int64_t y = p / W;
    const int x = (int)(p - y * W);
    const bool left = x > 0 && on[p - 1];
    if (left && (threadIdx.x & 63) == 0) uf_union(L, (int)p, (int)p - 1);
    if (y > 0) {
        const bool up = on[p - W] != 0, ul = x > 0 && on[p - W - 1];
        if (up && !(left && ul)) uf_union(L, (int)p, (int)p - W);
        if (CONN8) {
            const bool ur = x + 1 < W && on[p - W + 1];
            if (ul && !up && !left) uf_union(L, (int)p, (int)p - W - 1);
            if (ur && !up && !(x + 1 < W && on[p + 1])) uf_union(L, (int)p, (int)p - W + 1);
        }
    }
}

// every set pixel points at its root
__global__ __launch_bounds__(256) void flatten_kernel(const uint8_t *__restrict__ on, int64_t P, int *__restrict__ L) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P || !on[p]) return;
    const int r = uf_find(L, (int)p);
    if (r != (int)p) __atomic_store_n(&L[p], r, __ATOMIC_RELAXED);
}

// background labels that own a pixel of the page border are outside; i runs over the 2W + 2H border positions (corners twice)
__global__ __launch_bounds__(256) void mark_outside_kernel(const uint8_t *__restrict__ background, int H, int W, const int *__restrict__ L,
                                                           uint8_t *__restrict__ outside) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * W + 2 * H) return;
    int x, y;
    if (i < 2 * W) {
        x = i < W ? i : i - W;
        y = i < W ? 0 : H - 1;
    } else {
        const int j = i - 2 * W;
        y = j < H ? j : j - H;
        x = j < H ? 0 : W - 1;
    }
    const int64_t p = (int64_t)y * W + x;
    if (background[p]) outside[L[p]] = 1;
}

// background map -> filled map, in place: a pixel is filled unless it is background whose label reached the border
__global__ __launch_bounds__(256) void fill_kernel(uint8_t *__restrict__ on, int64_t P, const int *__restrict__ L,
                                                   const uint8_t *__restrict__ outside) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    on[p] = on[p] ? !outside[L[p]] : 1;
}

// Rectangle per root (x1 / y1 exclusive): only the pixels on a component's rim can move it — a pixel without a left / right / upper /
// lower neighbour of the map — so the solid inside of a blob issues no atomic at all.
__global__ __launch_bounds__(256) void boxes_kernel(const uint8_t *__restrict__ on, int H, int W, int64_t P, Planes pl) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P || !on[p]) return;
    const int r = pl.L[p];
    const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
    if (x == 0 || !on[p - 1]) atomicMin(&pl.x0[r], x);
    if (x + 1 >= W || !on[p + 1]) atomicMax(&pl.x1[r], x + 1);
    if (y == 0 || !on[p - W]) atomicMin(&pl.y0[r], y);
    if (y + 1 >= H || !on[p + W]) atomicMax(&pl.y1[r], y + 1);
}

// the roots go to the list, in any order: each is judged on its own.  At most one root per 2x2 block exists, the list holds P.
__global__ __launch_bounds__(256) void collect_kernel(const uint8_t *__restrict__ on, int64_t P, Planes pl) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool root = p < P && on[p] != 0 && pl.L[p] == (int)p;
    const int lane = threadIdx.x & 63;
    const unsigned long long rm = __ballot(root);
    if (!rm) return;
    int base = 0;
    if (lane == 0) base = atomicAdd(&pl.status[0], __popcll(rm));
    base = __shfl(base, 0);
    if (root) pl.list[base + __popcll(rm & ((1ull << lane) - 1ull))] = (int)p;
}

// sum_c (c - gray)^2 > 100 with gray = 0.299 r + 0.587 g + 0.114 b, in thousandths
__device__ __forceinline__ int is_coloured(int r, int g, int b) {
    const long long G = 299ll * r + 587ll * g + 114ll * b;
    const long long dr = 1000ll * r - G, dg = 1000ll * g - G, db = 1000ll * b - G;
    return dr * dr + dg * dg + db * db > 100000000ll;
}

__device__ __forceinline__ int wave_scan_inclusive(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}

// One wave per page row: inclusive prefix sums along the row of `coloured` and of the bright (> 127) elements that lie in the page's
// 2-pixel frame.  64 columns a step, the running totals carried in a register.
__global__ __launch_bounds__(256) void row_prefix_kernel(const uint8_t *__restrict__ page, int H, int W, int *__restrict__ sc,
                                                         int *__restrict__ sb) {
    const int y = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (y >= H) return;
    const bool frame_row = y < 2 || y >= H - 2;
    const uint8_t *row = page + (int64_t)y * W * 3;
    int carry_c = 0, carry_b = 0;
    for (int base = 0; base < W; base += 64) {
        const int x = base + lane;
        int c = 0, b = 0;
        if (x < W) {
            const int r = row[3 * (int64_t)x], g = row[3 * (int64_t)x + 1], bl = row[3 * (int64_t)x + 2];
            c = is_coloured(r, g, bl);
            if (frame_row || x < 2 || x >= W - 2) b = (r > 127) + (g > 127) + (bl > 127);
        }
        c = wave_scan_inclusive(c, lane) + carry_c;
        b = wave_scan_inclusive(b, lane) + carry_b;
        if (x < W) {
            sc[(int64_t)y * W + x] = c;
            sb[(int64_t)y * W + x] = b;
        }
        carry_c = __shfl(c, 63);
        carry_b = __shfl(b, 63);
    }
}

// One wave per component: the rectangle one pixel larger to the right and below, clamped to the page (cv2.rectangle's inclusive
// corners); erased when the dark share of the frame is inside [lo, hi] or more than 10 pixels are coloured.
__global__ __launch_bounds__(256) void decide_kernel(Planes pl, int H, int W, int total, int lo, int hi) {
    const int lane = threadIdx.x & 63;
    const int n = pl.status[0];
    for (int c = blockIdx.x * 4 + (threadIdx.x >> 6); c < n; c += gridDim.x * 4) {
        const int root = pl.list[c];
        const int xa = pl.x0[root], ya = pl.y0[root], xb = min(pl.x1[root] + 1, W), yb = min(pl.y1[root] + 1, H);   // xb / yb exclusive
        long long coloured = 0, bright = 0;
        for (int y = ya + lane; y < yb; y += 64) {
            const int64_t r = (int64_t)y * W;
            coloured += pl.sc[r + xb - 1] - (xa > 0 ? pl.sc[r + xa - 1] : 0);
            bright += pl.sb[r + xb - 1] - (xa > 0 ? pl.sb[r + xa - 1] : 0);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            coloured += __shfl_xor(coloured, o);
            bright += __shfl_xor(bright, o);
        }
        const long long dark = (long long)total - bright;
        if (lane == 0) pl.flag[root] = (lo <= dark && dark <= hi) || coloured > 10;
    }
}

__global__ __launch_bounds__(256) void erase_kernel(const uint8_t *__restrict__ on, int64_t P, const int *__restrict__ L,
                                                    const uint8_t *__restrict__ erase, uint8_t *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P || !on[p]) return;
    if (erase[L[p]]) out[p] = 0;
}

// One workgroup per line of a rectified chunk u8 [n, h, wp, 3].  lines: (w, lo, hi) per line.  dark: the elements <= 127 of the four
// numpy slices [0:2, 0:w], [h-2:h, 0:w], [2:h-2, 0:2], [2:h-2, w-2:w] — the last two overlap for w < 4 and such a pixel counts once
// per slice it lies in.  Columns >= w are not read.
__global__ __launch_bounds__(256) void crop_flags_kernel(uint8_t *__restrict__ region, int h, int wp, const int32_t *__restrict__ lines,
                                                         uint8_t *__restrict__ flags) {
    __shared__ int part[2][4];
    __shared__ int verdict;
    const int j = blockIdx.x;
    const int w = lines[3 * j], lo = lines[3 * j + 1], hi = lines[3 * j + 2];
    const int64_t row_bytes = (int64_t)h * wp * 3;
    uint8_t *base = region + j * row_bytes;
    if (w < 2 || w > wp) {   // not a line of this chunk: nothing read, nothing written but the flag
        if (threadIdx.x == 0) flags[j] = 2;
        return;
    }
    int dark = 0, coloured = 0;
    for (int i = threadIdx.x; i < h * w; i += blockDim.x) {
        const int y = i / w, x = i - y * w;
        const uint8_t *px = base + ((int64_t)y * wp + x) * 3;
        const int r = px[0], g = px[1], b = px[2];
        const int times = (y < 2) + (y >= h - 2) + ((y >= 2 && y < h - 2) ? (x < 2) + (x >= w - 2) : 0);
        dark += times * ((r <= 127) + (g <= 127) + (b <= 127));
        coloured += is_coloured(r, g, b);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        dark += __shfl_xor(dark, o);
        coloured += __shfl_xor(coloured, o);
    }
    if ((threadIdx.x & 63) == 0) part[0][threadIdx.x >> 6] = dark, part[1][threadIdx.x >> 6] = coloured;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int d = part[0][0] + part[0][1] + part[0][2] + part[0][3], c = part[1][0] + part[1][1] + part[1][2] + part[1][3];
        verdict = (lo <= d && d <= hi) || c > 10;
        flags[j] = (uint8_t)verdict;
    }
    __syncthreads();
    if (!verdict) return;
    // a rejected line's rows become zero, padding included: leading bytes up to a word boundary, whole words, trailing bytes
    const int64_t head = min((int64_t)((4 - (reinterpret_cast<uintptr_t>(base) & 3)) & 3), row_bytes);
    const int64_t words = (row_bytes - head) / 4, tail = head + 4 * words;
    if ((int64_t)threadIdx.x < head) base[threadIdx.x] = 0;
    uint32_t *wp32 = reinterpret_cast<uint32_t *>(base + head);
    for (int64_t i = threadIdx.x; i < words; i += blockDim.x) wp32[i] = 0u;
    if (tail + threadIdx.x < row_bytes) base[tail + threadIdx.x] = 0;
}

}  // namespace

extern "C" int64_t mit_bubble_filter_workspace_bytes(int H, int W) {
    if (H < 4 || W < 4 || (int64_t)H * W > INT32_MAX) return -1;
    const int64_t P = (int64_t)H * W;
    return STATUS_BYTES + INT_PLANES * P * (int64_t)sizeof(int) + BYTE_PLANES * P;
}

extern "C" int mit_bubble_filter(const uint8_t *mask_dev, const uint8_t *page_dev, int H, int W, int k, int lo, int hi, uint8_t *out_dev,
                                 void *ws_dev, int64_t ws_bytes, void *stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!mask_dev || !page_dev || !out_dev || !ws_dev) return mit_set_error("mit_bubble_filter: null pointer");
    if (H <= 0 || W <= 0) return mit_set_error("mit_bubble_filter: sizes must be positive (H %d W %d)", H, W);
    const int64_t need = mit_bubble_filter_workspace_bytes(H, W);
    if (need < 0) return mit_set_error("mit_bubble_filter: bad shape (H %d W %d): both sides at least 4, H * W below 2^31", H, W);
    if (k < 0 || k > (H > W ? H : W)) return mit_set_error("mit_bubble_filter: dilation size %d outside 0..max(H, W)", k);
    if (ws_bytes < need) return mit_set_error("mit_bubble_filter: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)need);
    if (reinterpret_cast<uintptr_t>(ws_dev) % 4) return mit_set_error("mit_bubble_filter: the workspace must be 4-byte aligned");
    const int64_t P = (int64_t)H * W;
    const Planes pl = carve(ws_dev, P);
    const int grid = mit_div_up(P, 256);
    const int kk = k > 0 ? k : 1;   // k == 0: no dilation, i.e. the one-tap maximum
    const int total = (int)(P - (int64_t)(H - 4) * (W - 4)) * 3;   // elements of the page's 2-pixel frame
    MitProbeScope probe("bubble_filter", stream, (double)P * (3 + 3 + 4 * 14));
    MIT_CHECK_HIP(hipMemsetAsync(pl.status, 0, STATUS_BYTES, stream));
    MIT_CHECK_HIP(hipMemsetAsync(pl.flag, 0, (size_t)P, stream));
    hipLaunchKernelGGL(row_max_kernel, dim3(grid), dim3(256), 0, stream, mask_dev, W, P, kk, pl.tmp);
    hipLaunchKernelGGL(col_max_kernel, dim3(grid), dim3(256), 0, stream, pl.tmp, H, W, P, kk, out_dev, pl.on);
    // holes: 4-connected background labels, the ones on the border are outside
    hipLaunchKernelGGL(init_kernel<false>, dim3(grid), dim3(256), 0, stream, pl.on, W, P, pl);
    hipLaunchKernelGGL(link_kernel<false>, dim3(grid), dim3(256), 0, stream, pl.on, W, P, pl.L);
    hipLaunchKernelGGL(flatten_kernel, dim3(grid), dim3(256), 0, stream, pl.on, P, pl.L);
    hipLaunchKernelGGL(mark_outside_kernel, dim3(mit_div_up(2 * (int64_t)W + 2 * (int64_t)H, 256)), dim3(256), 0, stream, pl.on, H, W, pl.L, pl.flag);
    hipLaunchKernelGGL(fill_kernel, dim3(grid), dim3(256), 0, stream, pl.on, P, pl.L, pl.flag);
    // components of the filled map, 8-connected
    hipLaunchKernelGGL(init_kernel<true>, dim3(grid), dim3(256), 0, stream, pl.on, W, P, pl);
    hipLaunchKernelGGL(link_kernel<true>, dim3(grid), dim3(256), 0, stream, pl.on, W, P, pl.L);
    hipLaunchKernelGGL(flatten_kernel, dim3(grid), dim3(256), 0, stream, pl.on, P, pl.L);
    hipLaunchKernelGGL(boxes_kernel, dim3(grid), dim3(256), 0, stream, pl.on, H, W, P, pl);
    hipLaunchKernelGGL(collect_kernel, dim3(grid), dim3(256), 0, stream, pl.on, P, pl);
    hipLaunchKernelGGL(row_prefix_kernel, dim3(mit_div_up(H, 4)), dim3(256), 0, stream, page_dev, H, W, pl.sc, pl.sb);
    hipLaunchKernelGGL(decide_kernel, dim3(grid < 1024 ? grid : 1024), dim3(256), 0, stream, pl, H, W, total, lo, hi);
    hipLaunchKernelGGL(erase_kernel, dim3(grid), dim3(256), 0, stream, pl.on, P, pl.L, pl.flag, out_dev);
    MIT_CHECK_LAUNCH("mit_bubble_filter");
    return 0;
}

extern "C" int mit_bubble_crop_flags(uint8_t *region_dev, int n, int h, int wp, const int32_t *lines_dev, uint8_t *flags_dev, void *stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!region_dev || !lines_dev || !flags_dev) return mit_set_error("mit_bubble_crop_flags: null pointer");
    if (n <= 0 || h <= 0 || wp <= 0) return mit_set_error("mit_bubble_crop_flags: sizes must be positive (n %d h %d wp %d)", n, h, wp);
    if (h < 4 || wp < 2) return mit_set_error("mit_bubble_crop_flags: bad shape (h %d wp %d): crops are at least 4 rows by 2 columns", h, wp);
    if ((int64_t)h * wp > INT32_MAX / 3) return mit_set_error("mit_bubble_crop_flags: a line of %d x %d pixels is too large", h, wp);
    MitProbeScope probe("bubble_crop_flags", stream, (double)n * h * wp * 3);
    hipLaunchKernelGGL(crop_flags_kernel, dim3(n), dim3(256), 0, stream, region_dev, h, wp, lines_dev, flags_dev);
    MIT_CHECK_LAUNCH("mit_bubble_crop_flags");
    return 0;
}
