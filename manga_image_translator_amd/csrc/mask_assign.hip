// mask_assign.hip — component labelling and text-line assignment of the mask refinement, on the device.
//
// Reference: manga_translator/mask_refinement/text_mask_utils.py:100-170 (the first half of complete_mask).  Device counterpart of
// mit_mask_assign_lines + mit_mask_line_crops (hostglue.hip) for a working-scale mask that already lives on the device: outline the
// lines' boxes with zeros, label the 8-connected components (lock-free union-find on the raster index, root = smallest index, as
// ctd_refine.hip / ctd_boxes.hip do), area and bounding rectangle per component with integer atomics on the root's slot, assign every
// component of more than 9 pixels to a text line by the host routine's rules, and paint the lines' component crops straight into the
// packed buffer mit_densecrf_refine reads.  Everything that decides is integer or is the host routine's own double / fp32 expression
// evaluated in the same order without contraction, so rectangles, crops and masks are equal to the host's, not close to them.
//
// Bounds: the page passes (init, link, flatten, stats, collect) each read or write a few int32 planes of H*W entries — HBM / atomic
// bound, ~10 us each at 1365x970; the assignment is one wave per component of more than 9 pixels with the lines spread over the lanes
// (fp64 latency bound, a few hundred components per page); the crop painter is one gather per output byte.
#include <math.h>
#include <stdint.h>
#include "../../include/mit_hip.h"
#include "common.h"

#pragma clang fp contract(off)  // the x86 host routine does not fuse: s1 - s2 of the shoelace sums and dp / (dp - dq) must round alike

namespace {

constexpr int PLANES = 7;  // L, area, x0, y0, x1, y1, assign
// A quad clipped by four half-planes: every pair of boundary crossings adds two vertices and drops at least one, and a line crosses
// an n-gon at most n times: 4 -> 6 -> 9 -> 13 -> 19 for the worst (self-intersecting) quad, 8 for a convex one.
constexpr int CLIP_CAP = 20;

struct Planes {
    int *L, *area, *x0, *y0, *x1, *y1, *asg, *list;
};

__host__ __device__ inline int64_t list_cap(int64_t P) { return P / 10 + 64; }

Planes carve(void *ws, int64_t P) {
    int *b = static_cast<int *>(ws);
    return Planes{b, b + P, b + 2 * P, b + 3 * P, b + 4 * P, b + 5 * P, b + 6 * P, b + 7 * P};
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

// cv2.rectangle(mask, (x, y), (x + w, y + h), 0, 1): one-pixel outline, inclusive corners, clipped, skipped when empty.  One block per line.
__global__ __launch_bounds__(256) void outline_kernel(uint8_t *__restrict__ mask, int H, int W, const int32_t *__restrict__ boxes) {
    const int i = blockIdx.x;
    const int64_t x = boxes[4 * i], y = boxes[4 * i + 1], w = boxes[4 * i + 2], h = boxes[4 * i + 3];
    const int64_t xa = x > 0 ? x : 0, xb = x + w < W - 1 ? x + w : W - 1, ya = y > 0 ? y : 0, yb = y + h < H - 1 ? y + h : H - 1;
    if (xa > xb || ya > yb) return;
    for (int s = 0; s < 2; ++s) {
        const int64_t yy = s ? y + h : y;
        if (yy >= 0 && yy < H)
            for (int64_t xx = xa + threadIdx.x; xx <= xb; xx += blockDim.x) mask[yy * W + xx] = 0;
        const int64_t xx = s ? x + w : x;
        if (xx >= 0 && xx < W)
            for (int64_t yy2 = ya + threadIdx.x; yy2 <= yb; yy2 += blockDim.x) mask[yy2 * W + xx] = 0;
    }
}

// The 64 pixels of a wave are consecutive in raster order: a horizontal run of mask pixels inside it (and inside one row) starts its
// life already linked to its first pixel, so link_kernel only joins runs across wave boundaries and rows.
__global__ __launch_bounds__(256) void init_kernel(const uint8_t *__restrict__ mask, int W, int64_t P, Planes pl) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool ok = p < P;
    const bool t = ok && mask[p] != 0;
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
    pl.area[p] = 0;
    pl.x0[p] = INT32_MAX;
    pl.y0[p] = INT32_MAX;
    pl.x1[p] = 0;
    pl.y1[p] = 0;
    pl.asg[p] = -1;
}

__global__ __launch_bounds__(256) void link_kernel(const uint8_t *__restrict__ mask, int W, int64_t P, int *__restrict__ L) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P || !mask[p]) return;
    const int64_t y = p / W;
    const int x = (int)(p - y * W);
    // Only the unions that can join two sets: (left) runs are pre-linked inside a wave, so only its first lane looks left; (up) not
    // when the left neighbour and the pixel above it are set too — the left neighbour makes that link; (diagonals) only when neither
    // the pixel above nor the horizontal neighbour below the diagonal can.
    const bool left = x > 0 && mask[p - 1];
    if (left && (threadIdx.x & 63) == 0) uf_union(L, (int)p, (int)p - 1);
    if (y > 0) {
        const bool up = mask[p - W] != 0, ul = x > 0 && mask[p - W - 1], ur = x + 1 < W && mask[p - W + 1];
        if (up && !(left && ul)) uf_union(L, (int)p, (int)p - W);
        if (ul && !up && !left) uf_union(L, (int)p, (int)p - W - 1);
        if (ur && !up && !(x + 1 < W && mask[p + 1])) uf_union(L, (int)p, (int)p - W + 1);
    }
}

// every pixel points at its root: the statistics, the crop painter and the host's tail find it in one step
__global__ __launch_bounds__(256) void flatten_kernel(const uint8_t *__restrict__ mask, int64_t P, int *__restrict__ L) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P || !mask[p]) return;
    const int r = uf_find(L, (int)p);
    if (r != (int)p) __atomic_store_n(&L[p], r, __ATOMIC_RELAXED);
}

// Area: one atomic per distinct root in the wave.  Rectangle: only the pixels on a component's rim can move it — a pixel without a
// left / right / upper / lower neighbour of the mask — so the solid inside of a blob issues no atomic at all.
__global__ __launch_bounds__(256) void stats_kernel(const uint8_t *__restrict__ mask, int H, int W, int64_t P, Planes pl) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool on = p < P && mask[p] != 0;
    int r = 0;
    if (on) {
        r = pl.L[p];
        const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
        if (x == 0 || !mask[p - 1]) atomicMin(&pl.x0[r], x);
        if (x + 1 >= W || !mask[p + 1]) atomicMax(&pl.x1[r], x + 1);
        if (y == 0 || !mask[p - W]) atomicMin(&pl.y0[r], y);
        if (y + 1 >= H || !mask[p + W]) atomicMax(&pl.y1[r], y + 1);
    }
    unsigned long long todo = __ballot(on);
    const int lane = threadIdx.x & 63;
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int k0 = __shfl(r, leader);
        const unsigned long long same = __ballot(on && r == k0);
        if (lane == leader) atomicAdd(&pl.area[k0], __popcll(same));
        todo &= ~same;
    }
}

// status[1]: number of components of more than 9 pixels (their roots go to the list, in any order: each is judged on its own);
// status[2]: number of components
__global__ __launch_bounds__(256) void collect_kernel(const uint8_t *__restrict__ mask, int64_t P, Planes pl, int *__restrict__ status) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool root = p < P && mask[p] != 0 && pl.L[p] == (int)p;
    const bool big = root && pl.area[p] > 9;
    const int lane = threadIdx.x & 63;
    const unsigned long long rm = __ballot(root), bm = __ballot(big);
    if (!rm) return;
    int base = 0;
    if (lane == 0) {
        atomicAdd(&status[2], __popcll(rm));
        if (bm) base = atomicAdd(&status[1], __popcll(bm));
    }
    base = __shfl(base, 0);
    if (big) pl.list[base + __popcll(bm & ((1ull << lane) - 1ull))] = (int)p;
}

struct Quad {
    double x[4], y[4];
};

__device__ __forceinline__ Quad load_quad(const double *__restrict__ polys, int i) {
    Quad q;
#pragma unroll
    for (int v = 0; v < 4; ++v) q.x[v] = polys[(int64_t)i * 8 + 2 * v], q.y[v] = polys[(int64_t)i * 8 + 2 * v + 1];
    return q;
}

__device__ __forceinline__ double quad_area(const Quad &q) {
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = (i + 1) & 3;
        s1 += q.x[i] * q.y[j];
        s2 += q.y[i] * q.x[j];
    }
    return fabs(s1 - s2) / 2;
}

// Area of quad ∩ [x0,x1] x [y0,y1] (Sutherland-Hodgman, the four sides in turn, then the shoelace sum): clip_poly_rect_area of
// hostglue.hip, statement for statement.  The two vertex lists live in LDS, one column per lane (vx / vy: [2][CLIP_CAP][64]), because
// lists indexed at run time in registers would become a private segment.
__device__ __forceinline__ double clip_quad_rect_area(const Quad &q, double x0, double y0, double x1, double y1, double *vx, double *vy, int lane) {
#define AT(list, i) ((((list) * CLIP_CAP) + (i)) * 64 + lane)
    int na = 4, cur = 0;
#pragma unroll
    for (int v = 0; v < 4; ++v) vx[AT(0, v)] = q.x[v], vy[AT(0, v)] = q.y[v];
    for (int side = 0; side < 4; ++side) {
        if (na == 0) return 0.0;
        const int axis = side >> 1;
        const double bound = side == 0 ? x0 : side == 1 ? x1 : side == 2 ? y0 : y1;
        const bool keep_ge = (side & 1) == 0;
        const int nxt = cur ^ 1;
        int nn = 0;
        for (int i = 0; i < na; ++i) {
            const int j = i + 1 == na ? 0 : i + 1;
            const double px = vx[AT(cur, i)], py = vy[AT(cur, i)], qx = vx[AT(cur, j)], qy = vy[AT(cur, j)];
            const double pc = axis ? py : px, qc = axis ? qy : qx;
            const double dp = keep_ge ? pc - bound : bound - pc, dq = keep_ge ? qc - bound : bound - qc;
            if (dp >= 0 && nn < CLIP_CAP) {
                vx[AT(nxt, nn)] = px, vy[AT(nxt, nn)] = py;
                ++nn;
            }
            if (((dp > 0 && dq < 0) || (dp < 0 && dq > 0)) && nn < CLIP_CAP) {
                const double t = dp / (dp - dq);
                vx[AT(nxt, nn)] = px + t * (qx - px), vy[AT(nxt, nn)] = py + t * (qy - py);
                ++nn;
            }
        }
        cur = nxt;
        na = nn;
    }
    if (na < 3) return 0.0;
    double s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < na; ++i) {
        const int j = i + 1 == na ? 0 : i + 1;
        s1 += vx[AT(cur, i)] * vy[AT(cur, j)];
        s2 += vy[AT(cur, i)] * vx[AT(cur, j)];
    }
    return fabs(s1 - s2) / 2;
#undef AT
}

// distance from a point to the quad (0 inside): poly_point_distance of hostglue.hip
__device__ __forceinline__ double quad_point_distance(const Quad &q, double px, double py) {
    bool inside = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = (i + 1) & 3;
        const double ax = q.x[i], ay = q.y[i], bx = q.x[j], by = q.y[j];
        if ((ay > py) != (by > py) && px < (bx - ax) * (py - ay) / (by - ay) + ax) inside = !inside;
    }
    if (inside) return 0.0;
    double best = INFINITY;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = (i + 1) & 3;
        const double ax = q.x[i], ay = q.y[i], bx = q.x[j], by = q.y[j];
        const double abx = bx - ax, aby = by - ay, den = abx * abx + aby * aby;
        double t = den == 0 ? 0.0 : ((px - ax) * abx + (py - ay) * aby) / den;
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
        const double dx = px - (ax + t * abx), dy = py - (ay + t * aby);
        const double d = sqrt(dx * dx + dy * dy);
        best = d < best ? d : best;  // std::min(best, d)
    }
    return best;
}

// One wave per component of more than 9 pixels; lane l looks at the lines l, l + 64, ...  A lane keeps its first maximum (`r > best`,
// so a NaN or a tie never replaces it) and the wave keeps the largest with the smallest line index: the line the host's serial loop
// ends with.  When no line beats the start value the host's index stays 0 and its ratio is line 0's own (a NaN): the same here.
__global__ __launch_bounds__(64) void assign_kernel(Planes pl, const double *__restrict__ polys, const double *__restrict__ font, int M,
                                                    double keep_threshold, int32_t *__restrict__ line_rects, int *__restrict__ status) {
    __shared__ double vx[2 * CLIP_CAP * 64], vy[2 * CLIP_CAP * 64];
    const int lane = threadIdx.x;
    const int n = status[1];
    for (int c = blockIdx.x; c < n; c += gridDim.x) {
        const int root = pl.list[c];
        const int area = pl.area[root];
        const int x1 = pl.x0[root], y1 = pl.y0[root], w1 = pl.x1[root] - x1, h1 = pl.y1[root] - y1;
        float best = -1.f, ratio0 = 0.f;
        int bi = INT32_MAX;
        for (int i = lane; i < M; i += 64) {
            const Quad q = load_quad(polys, i);
            double pminx = q.x[0], pmaxx = q.x[0], pminy = q.y[0], pmaxy = q.y[0];
#pragma unroll
            for (int v = 1; v < 4; ++v) {
                pminx = q.x[v] < pminx ? q.x[v] : pminx, pmaxx = pmaxx < q.x[v] ? q.x[v] : pmaxx;
                pminy = q.y[v] < pminy ? q.y[v] : pminy, pmaxy = pmaxy < q.y[v] ? q.y[v] : pmaxy;
            }
            float r = 0.f;
            if (pminx <= x1 + w1 && pmaxx >= x1 && pminy <= y1 + h1 && pmaxy >= y1) {
                const double a2 = quad_area(q), a1 = (double)area;
                r = (float)(clip_quad_rect_area(q, x1, y1, x1 + w1, y1 + h1, vx, vy, lane) / (a2 < a1 ? a2 : a1));
            }
            if (i == 0) ratio0 = r;
            if (r > best) best = r, bi = i;
        }
        ratio0 = __shfl(ratio0, 0);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o);
            const int oi = __shfl_xor(bi, o);
            if (ob > best || (ob == best && oi < bi)) best = ob, bi = oi;
        }
        int avg = bi == INT32_MAX ? 0 : bi;
        const float ratio_avg = bi == INT32_MAX ? ratio0 : best;
        if ((double)area >= quad_area(load_quad(polys, avg))) continue;
        if (ratio_avg <= (float)keep_threshold) {
            const double cx = x1 + w1 / 2.0, cy = y1 + h1 / 2.0;
            float dbest = INFINITY;
            int di = INT32_MAX;
            for (int i = lane; i < M; i += 64) {
                const float d = (float)quad_point_distance(load_quad(polys, i), cx, cy);
                if (d < dbest) dbest = d, di = i;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ob = __shfl_xor(dbest, o);
                const int oi = __shfl_xor(di, o);
                if (ob < dbest || (ob == dbest && oi < di)) dbest = ob, di = oi;
            }
            avg = di == INT32_MAX ? 0 : di;
            const double f = font[avg], fw = (double)w1 < f ? (double)w1 : f, fh = (double)h1 < fw ? (double)h1 : fw;
            const double unit = fh < 10.0 ? 10.0 : fh;  // max(min(min(font, w), h), 10)
            if ((double)dbest >= 0.5 * unit) continue;
        }
        if (lane == 0) {
            pl.asg[root] = avg;
            // coordinates are never negative: an unsigned minimum over 0xffffffff leaves the host's -1 in a line that got nothing
            atomicMin(reinterpret_cast<unsigned int *>(line_rects + 4 * avg), (unsigned int)x1);
            atomicMin(reinterpret_cast<unsigned int *>(line_rects + 4 * avg + 1), (unsigned int)y1);
            atomicMax(line_rects + 4 * avg + 2, x1 + w1);
            atomicMax(line_rects + 4 * avg + 3, y1 + h1);
            atomicAdd(&status[0], 1);
        }
    }
}

// out[offsets[j] + (yy * w + xx)] = 255 where pixel (x + xx, y + yy) belongs to a component assigned to job j's line
__global__ __launch_bounds__(256) void crops_kernel(const int *__restrict__ L, const int *__restrict__ asg, int H, int W,
                                                    const int32_t *__restrict__ jobs, const int64_t *__restrict__ offsets, int n_jobs,
                                                    int64_t total, uint8_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (offsets[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    const int line = jobs[5 * lo], x = jobs[5 * lo + 1], y = jobs[5 * lo + 2], w = jobs[5 * lo + 3], h = jobs[5 * lo + 4];
    const int64_t local = i - offsets[lo];
    uint8_t v = 0;
    if (line >= 0 && w > 0 && h > 0 && local >= 0 && local < (int64_t)w * h) {
        const int64_t yy = y + local / w, xx = x + local % w;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
            const int r = L[yy * W + xx];
            if (r >= 0 && asg[r] == line) v = 255;
        }
    }
    out[i] = v;
}

}  // namespace

extern "C" int64_t mit_mask_assign_workspace_bytes(int H, int W) {
    if (H <= 0 || W <= 0 || (int64_t)H * W > INT32_MAX) return -1;
    const int64_t P = (int64_t)H * W;
    return (PLANES * P + list_cap(P)) * (int64_t)sizeof(int);
}

extern "C" int mit_mask_assign_lines_dev(uint8_t *mask_dev, int H, int W, const int32_t *boxes_xywh_dev, const double *polys_dev,
                                         const double *font_size_dev, int M, int V, double keep_threshold, void *ws_dev, int64_t ws_bytes,
                                         int32_t *line_rects_dev, void *stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!mask_dev || !ws_dev || !line_rects_dev || (M > 0 && (!boxes_xywh_dev || !polys_dev || !font_size_dev)))
        return mit_set_error("mit_mask_assign_lines_dev: null pointer");
    if (V != 4) return mit_set_error("mit_mask_assign_lines_dev: quadrilaterals only (V %d); other polygons take mit_mask_assign_lines", V);
    const int64_t need = mit_mask_assign_workspace_bytes(H, W);
    if (need < 0 || M < 0) return mit_set_error("mit_mask_assign_lines_dev: bad shape (H %d W %d M %d)", H, W, M);
    if (ws_bytes < need) return mit_set_error("mit_mask_assign_lines_dev: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)need);
    const int64_t P = (int64_t)H * W;
    const Planes pl = carve(ws_dev, P);
    int *status = line_rects_dev + 4 * (int64_t)M;
    const int grid = mit_div_up(P, 256);
    MitProbeScope probe("mask_assign", stream, (double)P * (1 + 4 * PLANES));
    if (M > 0) MIT_CHECK_HIP(hipMemsetAsync(line_rects_dev, 0xff, sizeof(int32_t) * 4 * (size_t)M, stream));
    MIT_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int32_t) * 4, stream));
    if (M > 0) hipLaunchKernelGGL(outline_kernel, dim3(M), dim3(256), 0, stream, mask_dev, H, W, boxes_xywh_dev);
    hipLaunchKernelGGL(init_kernel, dim3(grid), dim3(256), 0, stream, mask_dev, W, P, pl);
    hipLaunchKernelGGL(link_kernel, dim3(grid), dim3(256), 0, stream, mask_dev, W, P, pl.L);
    hipLaunchKernelGGL(flatten_kernel, dim3(grid), dim3(256), 0, stream, mask_dev, P, pl.L);
    hipLaunchKernelGGL(stats_kernel, dim3(grid), dim3(256), 0, stream, mask_dev, H, W, P, pl);
    hipLaunchKernelGGL(collect_kernel, dim3(grid), dim3(256), 0, stream, mask_dev, P, pl, status);
    if (M > 0) {
        const int blocks = (int)(list_cap(P) < 2048 ? list_cap(P) : 2048);
        hipLaunchKernelGGL(assign_kernel, dim3(blocks), dim3(64), 0, stream, pl, polys_dev, font_size_dev, M, keep_threshold, line_rects_dev, status);
    }
    MIT_CHECK_LAUNCH("mit_mask_assign_lines_dev");
    return 0;
}

extern "C" int mit_mask_line_crops_dev(const void *ws_dev, int64_t ws_bytes, int H, int W, const int32_t *jobs_dev, const int64_t *offsets_dev,
                                       int n_jobs, int64_t total, uint8_t *out_dev, void *stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!ws_dev || (n_jobs > 0 && (!jobs_dev || !offsets_dev)) || (total > 0 && !out_dev))
        return mit_set_error("mit_mask_line_crops_dev: null pointer");
    const int64_t need = mit_mask_assign_workspace_bytes(H, W);
    if (need < 0 || n_jobs < 0 || total < 0) return mit_set_error("mit_mask_line_crops_dev: bad shape (H %d W %d, %d jobs, %lld bytes)", H, W, n_jobs, (long long)total);
    if (ws_bytes < need) return mit_set_error("mit_mask_line_crops_dev: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)need);
    if (total == 0 || n_jobs == 0) return 0;
    const int64_t P = (int64_t)H * W;
    const Planes pl = carve(const_cast<void *>(ws_dev), P);
    MitProbeScope probe("mask_line_crops", stream, (double)total * 9);
    hipLaunchKernelGGL(crops_kernel, dim3(mit_div_up(total, 256)), dim3(256), 0, stream, pl.L, pl.asg, H, W, jobs_dev, offsets_dev, n_jobs, total, out_dev);
    MIT_CHECK_LAUNCH("mit_mask_line_crops_dev");
    return 0;
}
