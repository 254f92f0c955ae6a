// ou_pool.hip -- the windowed enhance over a queue of clips (include/ouhip.h,
// "Windowed enhance"; DESIGN.md section 14, "Pooled windows"): the windows of
// several clips, all `window` samples long, share the groups of one (B, W)
// plan.
//
//  * ou_pool_slots        the arithmetic alone: N, the number of slots
//  * ou_pool_gather       fills a group's MIX rows and all its NZ rows
//  * ou_pool_overlap_add  crossfades a group's outputs into the clips' results
//
// The entry points keep no state: the clip list is a host array and every call
// works out its slots from it.  A launch gets its slots as a by-value table of
// at most kPoolSlots entries (read through the workgroup's uniform blockIdx.y);
// a larger group is several launches of the same call.  Nothing is allocated.
// Both kernels are plain HBM streams with 16-byte accesses where a row's
// address allows it (decided per row, uniform over a workgroup) and dword
// accesses otherwise.  Sample offsets are 64-bit; a window is an int.  Every
// store is a plain vector store.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ouhip.h"
#include "ou_common.h"

namespace {

constexpr int kPoolSlots = 32;   // slots per launch: the tables below travel as kernel arguments
constexpr long long kPoolMaxGrid = 0x7fffffffLL;

struct PoolGeom {
    long long N, hop;   // N: slots of the whole clip list
    int W, O;
};

inline long long pool_windows(long long T, const PoolGeom& g) { return 1 + (T - g.W + g.hop - 1) / g.hop; }

inline long long pool_start(long long T, long long i, const PoolGeom& g)
{
    const long long s = i * g.hop;
    return s < T - g.W ? s : T - g.W;
}

// the checks every entry point shares (T from the plain array or from the clip list); fills g
int pool_geom(const char* what, const int64_t* T, const ou_pool_clip* clips, int n_clips, int window, int overlap,
              PoolGeom* g)
{
    if (!T && !clips) return ou_fail(-1, "%s: null clip list", what);
    if (n_clips < 1) return ou_fail(-1, "%s: %d clips", what, n_clips);
    if (window <= 0 || overlap < 0) return ou_fail(-1, "%s: window %d, overlap %d", what, window, overlap);
    if (overlap > window / 2) return ou_fail(-1, "%s: overlap %d > window / 2 (%d)", what, overlap, window / 2);
    g->W = window;
    g->O = overlap;
    g->hop = window - overlap;
    g->N = 0;
    for (int c = 0; c < n_clips; ++c) {
        const long long Tc = T ? T[c] : clips[c].T;
        if (Tc <= window)
            return ou_fail(-1, "%s: clip %d has %lld samples, window %d (a clip that fits the window takes no slot)",
                           what, c, Tc, window);
        if (Tc > (1LL << 60) || g->N > (1LL << 61))
            return ou_fail(-1, "%s: clip %d has %lld samples after %lld slots", what, c, Tc, g->N);
        g->N += pool_windows(Tc, *g);
    }
    return 0;
}

// walks the slot list [(c, i) for c in order for i in range(n_c)] from slot `first`; a step past the last slot stays on it
struct PoolWalk {
    const ou_pool_clip* clips;
    const PoolGeom& g;
    int c;
    long long i, n, left;   // left: slots after this one
    PoolWalk(const ou_pool_clip* clips_, const PoolGeom& g_, long long first) : clips(clips_), g(g_), c(0), i(first)
    {
        left = g.N - 1 - first;
        for (n = pool_windows(clips[0].T, g); i >= n; n = pool_windows(clips[c].T, g)) i -= n, ++c;
    }
    long long start() const { return pool_start(clips[c].T, i, g); }
    void next()
    {
        if (left == 0) return;
        --left;
        if (++i == n) ++c, i = 0, n = pool_windows(clips[c].T, g);
    }
};

struct GatherSlot {
    const float* x;    // the window's first sample of the clip
    const float* nz;   // and of the clip's noise row 0
    long long nrs;     // the clip's noise row stride
};
struct GatherTable {
    GatherSlot s[kPoolSlots];
};

// grid (ceil(max(W, noise_win) / 1024), slots of the launch, 1 + noise_rows):
// z = 0 copies the slot's window of its clip to MIX, z = 1 + r the slice of
// its clip's noise row r to NZ.  4 values per lane: one 16-byte access where
// the row's base allows it.
__global__ void __launch_bounds__(256) pool_gather_kernel(GatherTable tab, int b0, int W, long long noise_win,
                                                          float* __restrict__ mix, long long mix_bstride,
                                                          float* __restrict__ nz, long long nz_rstride,
                                                          long long nz_bstride)
{
    const long long j = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    const long long r = (long long)blockIdx.z - 1;
    const long long win = r < 0 ? (long long)W : noise_win;
    if (j >= win) return;
    const GatherSlot& s = tab.s[blockIdx.y];
    const long long b = (long long)b0 + blockIdx.y;
    const float* src = r < 0 ? s.x + j : s.nz + r * s.nrs + j;
    float* dst = r < 0 ? mix + b * mix_bstride + j : nz + r * nz_rstride + b * nz_bstride + j;
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

struct AddSlot {
    float* y;                // the clip's result
    long long start, i, n;   // window i of the clip's n, starting at sample `start`
};
struct AddTable {
    AddSlot s[kPoolSlots];
};

// grid (ceil(W / 1024), slots of the launch): one thread per slot b of the
// call and four window-local samples j.  Sample t = start + j of the clip
// belongs to window own = min(t / H, n - 1) (ou_long.hip, long_sample).  The
// thread of the owning window stores the finished sample: outside the fade-in
// 0 + 1 v; inside it (0 + (1 - f) v_{i-1}) + f v_i, the first term taken from
// slot b - 1 when that is a slot of this call and from y[t], where the call
// of the group before left it, otherwise.  The thread of window own - 1 stores
// 0 + (1 - f) v only when the owner is not a slot of this call.  Everything
// else -- the discarded head of a shifted last window, the fade-out under an
// owner of the same call -- is written by nobody here, so no two threads of a
// call touch one sample, and once every group has run every sample of every
// clip has been stored by its owner.
__global__ void __launch_bounds__(256) pool_overlap_add_kernel(AddTable tab, long long b0, long long count, int W, int O,
                                                               const float* __restrict__ w, long long w_bstride,
                                                               const float* __restrict__ fade)
{
    const long long j0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (j0 >= W) return;
    const AddSlot& s = tab.s[blockIdx.y];
    const long long b = b0 + blockIdx.y, H = W - O, i = s.i;
    const bool prev_in = i > 0 && b > 0;                    // window i - 1 is slot b - 1 of this call
    const bool next_in = i + 1 < s.n && b + 1 < count;      // window i + 1 is slot b + 1 of this call
    const float* v = w + b * w_bstride + j0;
    const float* vp = w + (b - 1) * w_bstride;              // read only under prev_in
    float* y = s.y + s.start + j0;
    const bool whole = j0 + 4 <= W;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    if (whole && ((uintptr_t)v & 15) == 0) {
        const float4 q = *reinterpret_cast<const float4*>(v);
        a[0] = q.x, a[1] = q.y, a[2] = q.z, a[3] = q.w;
    } else {
        for (int k = 0; k < 4; ++k)
            if (j0 + k < W) a[k] = v[k];
    }
    long long t = s.start + j0, q = t / H, u = t - q * H;   // t = q H + u
    bool st[4] = {false, false, false, false};
    for (int k = 0; k < 4; ++k, ++t) {
        if (k && ++u == H) u = 0, ++q;
        if (j0 + k >= W) break;
        const long long own = q < s.n - 1 ? q : s.n - 1;
        const long long uo = t - own * H;                   // past the start of the owner's fade-in
        if (own == i) {
            if (i == 0 || uo >= O) {
                a[k] = __fadd_rn(0.f, __fmul_rn(1.f, a[k]));
            } else {
                // window i - 1 is not the shifted last one: it starts at (i - 1) H
                const float acc = prev_in ? __fadd_rn(0.f, __fmul_rn(fade[O + uo], vp[uo + H])) : y[k];
                a[k] = __fadd_rn(acc, __fmul_rn(fade[uo], a[k]));
            }
            st[k] = true;
        } else if (own == i + 1 && !next_in) {
            a[k] = __fadd_rn(0.f, __fmul_rn(fade[O + uo], a[k]));   // uo < O: window i ends at (i + 1) H + O
            st[k] = true;
        }
    }
    if (whole && st[0] && st[1] && st[2] && st[3] && ((uintptr_t)y & 15) == 0) {
        *reinterpret_cast<float4*>(y) = make_float4(a[0], a[1], a[2], a[3]);
    } else {
        for (int k = 0; k < 4; ++k)
            if (st[k]) y[k] = a[k];
    }
}

}  // namespace

extern "C" {

int ou_pool_slots(const int64_t* T, int n_clips, int window, int overlap, int64_t* n_slots)
{
    PoolGeom g;
    const int rc = pool_geom("pool_slots", T, nullptr, n_clips, window, overlap, &g);
    if (rc) return rc;
    if (n_slots) *n_slots = g.N;
    return 0;
}

int ou_pool_gather(const ou_pool_clip* clips, int n_clips, int window, int overlap, int64_t first, int count,
                   int noise_rows, int64_t noise_win, float* mix, int64_t mix_bstride, float* nz, int64_t nz_rstride,
                   int64_t nz_bstride, void* stream)
{
    PoolGeom g;
    const int rc = pool_geom("pool_gather", nullptr, clips, n_clips, window, overlap, &g);
    if (rc) return rc;
    if (!mix || (noise_rows > 0 && !nz)) return ou_fail(-1, "pool_gather: null destination");
    if (count < 1 || noise_rows < 0 || noise_rows > 65534 || (noise_rows > 0 && noise_win < 1))
        return ou_fail(-1, "pool_gather: count %d, noise rows %d, noise window %lld", count, noise_rows,
                       (long long)noise_win);
    if (first < 0 || first >= g.N) return ou_fail(-1, "pool_gather: first slot %lld of %lld", (long long)first, g.N);
    if (mix_bstride < window || (noise_rows > 0 && (nz_bstride < noise_win ||
                                                    nz_rstride < (long long)(count - 1) * nz_bstride + noise_win)))
        return ou_fail(-1, "pool_gather: rows or items overlap (strides %lld, %lld, %lld)", (long long)mix_bstride,
                       (long long)nz_rstride, (long long)nz_bstride);
    for (int c = 0; c < n_clips; ++c) {
        if (!clips[c].x || (noise_rows > 0 && !clips[c].noise)) return ou_fail(-1, "pool_gather: clip %d: null", c);
        if (noise_rows > 0 && clips[c].noise_rstride < clips[c].T - window + noise_win)
            return ou_fail(-1, "pool_gather: clip %d: noise rows of %lld values, %lld needed", c,
                           (long long)clips[c].noise_rstride, (long long)(clips[c].T - window + noise_win));
    }
    const long long wmax = noise_rows > 0 && noise_win > window ? (long long)noise_win : (long long)window;
    const long long gx = (wmax + 1023) / 1024;
    if (gx > kPoolMaxGrid) return ou_fail(-1, "pool_gather: window %lld is too long", wmax);
    PoolWalk at(clips, g, first);
    for (int b0 = 0; b0 < count; b0 += kPoolSlots) {
        const int nb = count - b0 < kPoolSlots ? count - b0 : kPoolSlots;
        GatherTable tab = {};
        for (int k = 0; k < nb; ++k, at.next()) {   // past the last slot the walk stays on it: the clamp
            const ou_pool_clip& cl = clips[at.c];
            tab.s[k].x = cl.x + at.start();
            tab.s[k].nz = noise_rows > 0 ? cl.noise + at.start() : nullptr;
            tab.s[k].nrs = cl.noise_rstride;
        }
        hipLaunchKernelGGL(pool_gather_kernel, dim3((unsigned)gx, (unsigned)nb, (unsigned)(1 + noise_rows)), dim3(256),
                           0, (hipStream_t)stream, tab, b0, window, (long long)noise_win, mix, (long long)mix_bstride,
                           nz, (long long)nz_rstride, (long long)nz_bstride);
        const int lrc = ou_check_launch("pool_gather");
        if (lrc) return lrc;
    }
    return 0;
}

int ou_pool_overlap_add(const ou_pool_clip* clips, int n_clips, int window, int overlap, int64_t first, int count,
                        const float* w, int64_t w_bstride, const float* fade, void* stream)
{
    PoolGeom g;
    const int rc = pool_geom("pool_overlap_add", nullptr, clips, n_clips, window, overlap, &g);
    if (rc) return rc;
    if (!w) return ou_fail(-1, "pool_overlap_add: null");
    if (overlap > 0 && !fade) return ou_fail(-1, "pool_overlap_add: no fade table for overlap %d", overlap);
    if (count < 1 || w_bstride < window)
        return ou_fail(-1, "pool_overlap_add: count %d, stride %lld", count, (long long)w_bstride);
    if (first < 0 || first >= g.N)
        return ou_fail(-1, "pool_overlap_add: first slot %lld of %lld", (long long)first, g.N);
    for (int c = 0; c < n_clips; ++c) {
        if (!clips[c].y) return ou_fail(-1, "pool_overlap_add: clip %d: null", c);
        // a clip's own fade-ins read what an earlier group stored: results may not share samples
        for (int d = 0; d < c; ++d) {
            const uintptr_t a0 = (uintptr_t)clips[c].y, a1 = a0 + (uintptr_t)clips[c].T * 4;
            const uintptr_t b0 = (uintptr_t)clips[d].y, b1 = b0 + (uintptr_t)clips[d].T * 4;
            if (a0 < b1 && b0 < a1) return ou_fail(-1, "pool_overlap_add: the results of clips %d and %d overlap", d, c);
        }
    }
    const long long gx = ((long long)window + 1023) / 1024;
    // slots at and past N repeat the last window; their outputs are dropped
    const long long n = g.N - first < count ? g.N - first : (long long)count;
    PoolWalk at(clips, g, first);
    for (long long b0 = 0; b0 < n; b0 += kPoolSlots) {
        const int nb = n - b0 < kPoolSlots ? (int)(n - b0) : kPoolSlots;
        AddTable tab = {};
        for (int k = 0; k < nb; ++k, at.next()) {
            tab.s[k].y = clips[at.c].y;
            tab.s[k].start = at.start();
            tab.s[k].i = at.i;
            tab.s[k].n = at.n;
        }
        hipLaunchKernelGGL(pool_overlap_add_kernel, dim3((unsigned)gx, (unsigned)nb), dim3(256), 0,
                           (hipStream_t)stream, tab, b0, n, window, overlap, w, (long long)w_bstride, fade);
        const int lrc = ou_check_launch("pool_overlap_add");
        if (lrc) return lrc;
    }
    return 0;
}

}  // extern "C"
