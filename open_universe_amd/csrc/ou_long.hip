// ou_long.hip -- the two kernels around the windowed enhance of a long clip
// (include/ouhip.h, "Windowed enhance"):
//
//  * ou_window_gather  copies a group's windows of the clip, or of the global
//                      noise, into the plan's batch buffers
//  * ou_overlap_add    crossfades a group's outputs into the clip's result
//
// Both are plain HBM streams, run once per group around the replay of the
// recorded plan.  A window starts at any sample, so a row is copied with
// 16-byte accesses only when its first address allows it (checked per row, on
// the device; the check is uniform over a workgroup) and with dword accesses
// otherwise.  Sample offsets are 64-bit throughout: a clip may pass 2^31
// samples, a window may not (int).  Every store is a plain vector store.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/ouhip.h"
#include "ou_common.h"

namespace {

struct LongGeom {
    long long T, n, hop, last;   // last = T - W, the start of the shifted last window
    int W, O;
};

// the checks every entry point shares; fills g
int long_geom(const char* what, int64_t T, int window, int overlap, LongGeom* g)
{
    if (window <= 0 || overlap < 0) return ou_fail(-1, "%s: window %d, overlap %d", what, window, overlap);
    if (overlap > window / 2) return ou_fail(-1, "%s: overlap %d > window / 2 (%d)", what, overlap, window / 2);
    if (T < 1 || T < window) return ou_fail(-1, "%s: clip of %lld samples, window %d", what, (long long)T, window);
    g->T = T;
    g->W = window;
    g->O = overlap;
    g->hop = window - overlap;
    g->last = T - window;
    g->n = 1 + (g->last + g->hop - 1) / g->hop;
    return 0;
}

__host__ __device__ __forceinline__ long long win_start(const LongGeom& g, long long i)
{
    const long long k = i < g.n - 1 ? i : g.n - 1;
    const long long s = k * g.hop;
    return s < g.last ? s : g.last;
}

// 4 values per lane: one 16-byte access where the row's base allows it
__global__ void __launch_bounds__(256) window_gather_kernel(const float* __restrict__ x, long long x_rstride, LongGeom g,
                                                            long long first, long long win, float* __restrict__ y,
                                                            long long y_rstride, long long y_bstride)
{
    const long long j = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (j >= win) return;
    const long long b = blockIdx.y, r = blockIdx.z;
    const float* src = x + r * x_rstride + win_start(g, first + b) + j;
    float* dst = y + r * y_rstride + b * y_bstride + j;
    const bool whole = j + 4 <= win;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (whole && ((uintptr_t)src & 15) == 0) {
        const float4 q = *reinterpret_cast<const float4*>(src);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
        for (int k = 0; k < 4; ++k)
            if (j + k < win) v[k] = src[k];
    }
    if (whole && ((uintptr_t)dst & 15) == 0) {
        *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int k = 0; k < 4; ++k)
            if (j + k < win) dst[k] = v[k];
    }
}

// One output sample: the contributions of the (at most two) windows of
// [first, first + count) that are non-zero at t, added to acc in window order.
// Sample t belongs to window i = min(t / H, n - 1): for 1 <= i <= n - 1 the
// fade-in of window i starts at e(i-1) - O = i H (only the last window is
// shifted, and it starts at or before (n - 1) H).
__device__ __forceinline__ bool long_sample(const float* __restrict__ w, long long w_bstride, const LongGeom& g,
                                            long long first, int count, const float* __restrict__ fade, long long t,
                                            float& acc)
{
    long long i = t / g.hop;
    if (i > g.n - 1) i = g.n - 1;
    bool any = false;
    float wi = 1.f;
    if (i >= 1) {
        const long long u = t - i * g.hop;
        if (u < g.O) {
            wi = fade[u];
            const long long p = i - 1;
            if (p >= first && p < first + count) {
                const float v = w[(p - first) * w_bstride + (t - win_start(g, p))];
                acc = __fadd_rn(acc, __fmul_rn(fade[g.O + u], v));
                any = true;
            }
        }
    }
    if (i >= first && i < first + count) {
        const float v = w[(i - first) * w_bstride + (t - win_start(g, i))];
        acc = __fadd_rn(acc, __fmul_rn(wi, v));
        any = true;
    }
    return any;
}

// kVec: y is 16-byte aligned (one float4 per lane); the call with first = 0
// starts every sample from 0 and stores all of them.  The launch covers
// samples [t_begin, t_end), t_begin a multiple of 4: the whole clip for
// first = 0, else the span in which the call's windows are non-zero.
template <bool kVec>
__global__ void __launch_bounds__(256) overlap_add_kernel(const float* __restrict__ w, long long w_bstride, LongGeom g,
                                                          long long first, int count, const float* __restrict__ fade,
                                                          float* __restrict__ y, long long t_begin, long long t_end)
{
    const long long t0 = t_begin + ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (t0 >= t_end) return;
    const bool clear = first == 0;
    if (kVec && t0 + 4 <= g.T) {
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!clear) q = *reinterpret_cast<const float4*>(y + t0);
        float a[4] = {q.x, q.y, q.z, q.w};
        bool any = clear;
        for (int k = 0; k < 4; ++k) any = long_sample(w, w_bstride, g, first, count, fade, t0 + k, a[k]) || any;
        if (any) *reinterpret_cast<float4*>(y + t0) = make_float4(a[0], a[1], a[2], a[3]);
    } else {
        for (int k = 0; k < 4; ++k) {
            const long long t = t0 + k;
            if (t >= g.T) break;
            float a = clear ? 0.f : y[t];
            if (long_sample(w, w_bstride, g, first, count, fade, t, a) || clear) y[t] = a;
        }
    }
}

constexpr long long kMaxGrid = 0x7fffffffLL;

}  // namespace

extern "C" {

int ou_long_windows(int64_t T, int window, int overlap, int64_t* n, int64_t* last_start)
{
    LongGeom g;
    const int rc = long_geom("long_windows", T, window, overlap, &g);
    if (rc) return rc;
    if (n) *n = g.n;
    if (last_start) *last_start = g.last;
    return 0;
}

int ou_long_fade(int overlap, float* fade)
{
    if (overlap < 0 || (overlap > 0 && !fade)) return ou_fail(-1, "long_fade: bad args");
    const double pi = 3.14159265358979323846;
    for (int u = 0; u < overlap; ++u) {
        const double s = std::sin(pi * (2.0 * u + 1.0) / (4.0 * overlap));
        fade[u] = (float)(s * s);
        fade[overlap + u] = (float)(1.0 - s * s);
    }
    return 0;
}

int ou_window_gather(const float* x, int64_t x_rstride, int rows, int64_t T, int window, int overlap,
                     int64_t first, int count, int64_t win, float* y, int64_t y_rstride, int64_t y_bstride,
                     void* stream)
{
    if (!x || !y) return ou_fail(-1, "window_gather: null");
    LongGeom g;
    const int rc = long_geom("window_gather", T, window, overlap, &g);
    if (rc) return rc;
    if (rows <= 0 || rows > 65535 || count <= 0 || count > 65535 || win <= 0)
        return ou_fail(-1, "window_gather: rows %d, count %d, win %lld", rows, count, (long long)win);
    if (first < 0 || first >= g.n)
        return ou_fail(-1, "window_gather: first window %lld of %lld", (long long)first, g.n);
    if (y_bstride < win || (rows > 1 && (x_rstride < g.last + win || y_rstride < (count - 1) * y_bstride + win)))
        return ou_fail(-1, "window_gather: rows or items overlap (strides %lld, %lld, %lld)", (long long)x_rstride,
                       (long long)y_rstride, (long long)y_bstride);
    const long long gx = (win + 1023) / 1024;
    if (gx > kMaxGrid) return ou_fail(-1, "window_gather: win %lld is too long", (long long)win);
    hipLaunchKernelGGL(window_gather_kernel, dim3((unsigned)gx, (unsigned)count, (unsigned)rows), dim3(256), 0,
                       (hipStream_t)stream, x, (long long)x_rstride, g, (long long)first, (long long)win, y,
                       (long long)y_rstride, (long long)y_bstride);
    return ou_check_launch("window_gather");
}

int ou_overlap_add(const float* w, int64_t w_bstride, int64_t T, int window, int overlap, int64_t first,
                   int count, const float* fade, float* y, void* stream)
{
    if (!w || !y) return ou_fail(-1, "overlap_add: null");
    LongGeom g;
    const int rc = long_geom("overlap_add", T, window, overlap, &g);
    if (rc) return rc;
    if (overlap > 0 && !fade) return ou_fail(-1, "overlap_add: no fade table for overlap %d", overlap);
    if (count <= 0 || w_bstride < window)
        return ou_fail(-1, "overlap_add: count %d, stride %lld", count, (long long)w_bstride);
    if (first < 0 || first >= g.n) return ou_fail(-1, "overlap_add: first window %lld of %lld", (long long)first, g.n);
    // A later call touches only the samples where its windows are non-zero:
    // from the fade-in of window `first` (at first H) to the end of its last
    // window, so the groups of a clip read and write O(T) in total.  The
    // first call writes the whole clip.
    long long last_w = first + count - 1;
    if (last_w > g.n - 1) last_w = g.n - 1;
    const long long t_begin = first == 0 ? 0 : (first * g.hop) & ~3LL;
    const long long t_end = first == 0 ? (long long)T : win_start(g, last_w) + g.W;
    const long long gx = (t_end - t_begin + 1023) / 1024;
    if (gx > kMaxGrid) return ou_fail(-1, "overlap_add: clip of %lld samples is too long", (long long)T);
    if ((uintptr_t)y % 16 == 0)
        hipLaunchKernelGGL(overlap_add_kernel<true>, dim3((unsigned)gx), dim3(256), 0, (hipStream_t)stream, w,
                           (long long)w_bstride, g, (long long)first, count, fade, y, t_begin, t_end);
    else
        hipLaunchKernelGGL(overlap_add_kernel<false>, dim3((unsigned)gx), dim3(256), 0, (hipStream_t)stream, w,
                           (long long)w_bstride, g, (long long)first, count, fade, y, t_begin, t_end);
    return ou_check_launch("overlap_add");
}

}  // extern "C"
