// ou_stream.hip -- the two kernels around a streaming enhance (include/ouhip.h,
// "Streaming enhance"): a stream is the windowed enhance
// of section 14 on everything pushed so far, run window by window as the
// samples arrive.
//
//  * ou_stream_gather       fills a group's MIX rows from the input ring and
//                           generates all its NZ rows in place
//  * ou_stream_overlap_add  emits the samples a group makes final, crossfaded
//                           with the carried tail of the window before it
//
// The entry points keep no state and allocate nothing: the ring, the carry and
// the counts of samples fed and windows run are the caller's (ou_model_stream_*
// in ou_model.hip, Universe.stream in Python).  A launch gets its slots' starts
// as a by-value table of at most kStreamSlots entries; a larger group is
// several launches of the same call.  Sample positions are 64-bit; a window is
// an int.  Every store is a plain vector store.
//
// ou_mux.hip includes this file with OU_STREAM_SHARED_ONLY defined and gets the
// part both share -- the geometry checks and stream_emit_quad, the per-sample
// rule of the overlap-add -- without the kernels and entry points below it.
// (tests/test_emu_stream.py builds a copy of this file beside ou_common.h,
// ou_normal.h and ou_philox.h alone, so the shared part lives here and not in
// a header of its own.)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/ouhip.h"
#include "ou_common.h"
#include "ou_normal.h"

namespace {

constexpr int kStreamSlots = 32;   // slots per launch: the table below travels as a kernel argument
constexpr long long kStreamMaxGrid = 0x7fffffffLL;
constexpr long long kStreamMaxSamples = 1LL << 40;   // per draw: 2^38 Philox counters of four samples

struct StreamGeom {
    long long hop, first, T;   // T: the stream's length, read only when closing
    int W, O, count, closing;
};

// the checks both entry points share; fills g
int stream_geom(const char* what, int window, int overlap, int64_t first, int count, int closing, int64_t T,
                StreamGeom* g)
{
    if (window <= 0 || overlap < 0) return ou_fail(-1, "%s: window %d, overlap %d", what, window, overlap);
    if (overlap > window / 2) return ou_fail(-1, "%s: overlap %d > window / 2 (%d)", what, overlap, window / 2);
    const long long hop = window - overlap;
    if (first < 0 || count < 0 || first > kStreamMaxSamples / hop)
        return ou_fail(-1, "%s: first window %lld, count %d", what, (long long)first, count);
    if (!closing) {
        if (count < 1) return ou_fail(-1, "%s: count %d", what, count);
    } else {
        if (T < window) return ou_fail(-1, "%s: a stream of %lld samples is shorter than one window of %d", what,
                                       (long long)T, window);
        if (T > kStreamMaxSamples) return ou_fail(-1, "%s: a stream of %lld samples passes 2^40", what, (long long)T);
        const long long n = 1 + (T - window + hop - 1) / hop;
        if (first + count != n || (count == 0 && T != (n - 1) * hop + window))
            return ou_fail(-1, "%s: closing at %lld samples with windows [%lld, %lld): the stream has %lld windows%s",
                           what, (long long)T, (long long)first, (long long)first + count, n,
                           count == 0 ? ", the last of them shifted" : "");
    }
    g->hop = hop;
    g->first = first;
    g->T = closing ? T : 0;
    g->W = window;
    g->O = overlap;
    g->count = count;
    g->closing = closing ? 1 : 0;
    return 0;
}

// start of window first + b, b < count: only the last window of a closing call is shifted back to end at T
__host__ __device__ __forceinline__ long long stream_start(const StreamGeom& g, long long b)
{
    const long long s = (g.first + b) * g.hop;
    return g.closing && b == g.count - 1 && s > g.T - g.W ? g.T - g.W : s;
}

// Four output samples of one stream: out[m .. m + 3] are the samples t = first H
// + m .. of the stream, t < t_end; w is the stream's first slot of this call,
// carry its carry.  stream_overlap_add_kernel below states the rule; this is
// its body, shared with mux_overlap_add_kernel (ou_mux.hip), which runs it once
// per run of a channel's slots.
__device__ __forceinline__ void stream_emit_quad(const float* __restrict__ w, long long w_bstride, const StreamGeom& g,
                                                 const float* __restrict__ fade, float* __restrict__ carry,
                                                 float* __restrict__ out, long long t_end, long long m)
{
    const long long t0 = g.first * g.hop;
    if (t0 + m >= t_end) return;
    const long long last = g.first + g.count - 1;
    const long long last_start = g.count > 0 ? stream_start(g, g.count - 1) : 0;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    int nv = 0;
    long long t = t0 + m, q = t / g.hop, u = t - q * g.hop;   // t = q H + u
    for (int k = 0; k < 4; ++k, ++t) {
        if (k && ++u == g.hop) u = 0, ++q;
        if (t >= t_end) break;
        const long long own = q < last ? q : last;
        const long long uo = t - own * g.hop;                 // past the start of the owner's fade-in
        if (own < g.first) {
            a[k] = fmaf(1.f, carry[m + k], 0.f);   // count = 0: t - t0 < O
        } else {
            const float v = w[(own - g.first) * w_bstride + (t - (own == last ? last_start : own * g.hop))];
            if (own >= 1 && uo < g.O) {
                const float vp = own == g.first ? carry[uo] : w[(own - 1 - g.first) * w_bstride + uo + g.hop];
                a[k] = fmaf(fade[uo], v, fmaf(fade[g.O + uo], vp, 0.f));
            } else {
                a[k] = fmaf(1.f, v, 0.f);
            }
        }
        nv = k + 1;
    }
    if (nv == 4 && ((uintptr_t)(out + m) & 15) == 0) {
        *reinterpret_cast<float4*>(out + m) = make_float4(a[0], a[1], a[2], a[3]);
    } else {
        for (int k = 0; k < nv; ++k) out[m + k] = a[k];
    }
    if (!g.closing)
        for (int k = 0; k < 4; ++k)
            if (m + k < g.O) carry[m + k] = w[(long long)(g.count - 1) * w_bstride + g.hop + m + k];
}

#ifndef OU_STREAM_SHARED_ONLY

struct StreamTable {
    long long s[kStreamSlots];
};

// grid (lanes / 256, slots of the launch, 1 + noise_rows).
// z = 0 copies the slot's window of the ring to MIX, four samples per lane; the
// ring holds position p at p mod cap, so a lane's four may wrap.
// z = 1 + r generates noise row r: a lane owns one counter of the global
// stream, q = (s >> 2) + lane, whose four normals are the samples 4 q .. 4 q + 3
// of the draw; they land at j0 = 4 q - s in the row, -4 < j0, so the first and
// the last lane of a row may hold fewer than four of its values.
__global__ void __launch_bounds__(256) stream_gather_kernel(StreamTable tab, int b0, const float* __restrict__ ring,
                                                            long long cap, int W, long long noise_win, uint32_t k0,
                                                            uint32_t k1, unsigned long long offset,
                                                            float* __restrict__ mix, long long mix_bstride,
                                                            float* __restrict__ nz, long long nz_rstride,
                                                            long long nz_bstride)
{
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long s = tab.s[blockIdx.y];
    const long long b = (long long)b0 + blockIdx.y;
    if (blockIdx.z == 0) {
        const long long j = lane * 4;
        if (j >= W) return;
        const long long p = (s + j) % cap;
        float* dst = mix + b * mix_bstride + j;
        const bool whole = j + 4 <= W;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (whole && p + 4 <= cap && ((uintptr_t)(ring + p) & 15) == 0) {
            const float4 q = *reinterpret_cast<const float4*>(ring + p);
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        } else {
            for (int k = 0; k < 4; ++k)
                if (j + k < W) v[k] = ring[p + k < cap ? p + k : p + k - cap];
        }
        if (whole && ((uintptr_t)dst & 15) == 0) {
            *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            for (int k = 0; k < 4; ++k)
                if (j + k < W) dst[k] = v[k];
        }
        return;
    }
    const long long r = (long long)blockIdx.z - 1;
    const long long q = (s >> 2) + lane;
    const long long j0 = 4 * q - s;
    if (j0 >= noise_win) return;
    float z[4];
    ouhip_detail::normal4(k0, k1, offset + ((unsigned long long)r << 38) + (unsigned long long)q, z);
    float* row = nz + r * nz_rstride + b * nz_bstride;
    const bool head = j0 < 0;                  // the row starts inside this counter
    const bool tail = j0 + 4 > noise_win;      // the row ends inside this counter
    if (!head && !tail && ((uintptr_t)(row + j0) & 15) == 0) {
        *reinterpret_cast<float4*>(row + j0) = make_float4(z[0], z[1], z[2], z[3]);
    } else {
        for (int k = 0; k < 4; ++k)
            if (j0 + k >= 0 && j0 + k < noise_win) row[j0 + k] = z[k];
    }
}

// One thread per four output samples: out[m] is sample t = first H + m of the
// stream, t < t_end.  Sample t belongs to window own = min(t / H, last) with
// last = first + count - 1 the last window there is for it (ou_long.hip,
// long_sample): outside the owner's fade-in 0 + 1 v, inside it
// (0 + (1 - f) v_{own-1}) + f v_own, where v_{own-1} comes from the slot before
// when that is a slot of this call and from the carry -- the raw last O samples
// of window first - 1 -- when own = first.  A closing call without windows emits
// the carry with weight 1.  Each "+ w v" is one fused multiply-add, written as
// fmaf: that is what ou_overlap_add's acc + w v is on the device (hipcc
// contracts it, __fadd_rn and __fmul_rn being a plain sum and product there),
// and the stream must give its bits; a sum of two separately rounded products
// differs from it in the last place at a few samples of every fade.  The thread
// that reads carry[u] is the one that then stores the next carry there (u = m <
// O <= H <= count H), the raw tail of this call's last window, so no two threads
// touch one word of the carry or of out.
__global__ void __launch_bounds__(256) stream_overlap_add_kernel(const float* __restrict__ w, long long w_bstride,
                                                                 StreamGeom g, const float* __restrict__ fade,
                                                                 float* __restrict__ carry, float* __restrict__ out,
                                                                 long long t_end)
{
    stream_emit_quad(w, w_bstride, g, fade, carry, out, t_end, ((long long)blockIdx.x * 256 + threadIdx.x) * 4);
}

#endif  // OU_STREAM_SHARED_ONLY

}  // namespace

#ifndef OU_STREAM_SHARED_ONLY

extern "C" {

int ou_stream_gather(const float* ring, int64_t cap, int64_t lo, int64_t fed, int window, int overlap, int64_t first,
                     int count, int slots, int closing, int64_t T, int noise_rows, int64_t noise_win, uint64_t seed,
                     uint64_t offset, float* mix, int64_t mix_bstride, float* nz, int64_t nz_rstride,
                     int64_t nz_bstride, void* stream)
{
    StreamGeom g;
    const int rc = stream_geom("stream_gather", window, overlap, first, count, closing, T, &g);
    if (rc) return rc;
    if (!ring || !mix || (noise_rows > 0 && !nz)) return ou_fail(-1, "stream_gather: null");
    if (count < 1 || slots < count || slots > 65535 || noise_rows < 0 || noise_rows > 65534 ||
        (noise_rows > 0 && noise_win < 1))
        return ou_fail(-1, "stream_gather: count %d, slots %d, noise rows %d, noise window %lld", count, slots,
                       noise_rows, (long long)noise_win);
    if (cap < window || lo < 0 || fed < lo || fed - lo > cap || fed > kStreamMaxSamples)
        return ou_fail(-1, "stream_gather: a ring of %lld samples holding [%lld, %lld), window %d", (long long)cap,
                       (long long)lo, (long long)fed, window);
    if (closing && T != fed)
        return ou_fail(-1, "stream_gather: closing at %lld samples, %lld fed", (long long)T, (long long)fed);
    if (((uintptr_t)ring | (uintptr_t)mix | (uintptr_t)nz) % 4)
        return ou_fail(-1, "stream_gather: a buffer is not aligned to a float");
    if (mix_bstride < window || (noise_rows > 0 && (nz_bstride < noise_win ||
                                                    nz_rstride < (long long)(slots - 1) * nz_bstride + noise_win)))
        return ou_fail(-1, "stream_gather: rows or items overlap (strides %lld, %lld, %lld)", (long long)mix_bstride,
                       (long long)nz_rstride, (long long)nz_bstride);
    for (int b = 0; b < count; ++b) {
        const long long s = stream_start(g, b);
        if (s < lo || s + window > fed)
            return ou_fail(-1, "stream_gather: window %lld covers [%lld, %lld), the ring holds [%lld, %lld)",
                           (long long)first + b, s, s + window, (long long)lo, (long long)fed);
        if (noise_rows > 0 && s + noise_win > kStreamMaxSamples)
            return ou_fail(-1, "stream_gather: window %lld draws noise past sample 2^40", (long long)first + b);
    }
    const long long wl = ((long long)window + 3) / 4;
    const long long nl = noise_rows > 0 ? ((long long)noise_win + 3) / 4 + 1 : 0;   // counters a row can touch
    const long long gx = ((wl > nl ? wl : nl) + 255) / 256;
    if (gx > kStreamMaxGrid) return ou_fail(-1, "stream_gather: window %lld is too long", (long long)noise_win);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int b0 = 0; b0 < slots; b0 += kStreamSlots) {
        const int nb = slots - b0 < kStreamSlots ? slots - b0 : kStreamSlots;
        StreamTable tab = {};
        for (int k = 0; k < nb; ++k)   // the slots past the real windows repeat the last of them
            tab.s[k] = stream_start(g, b0 + k < count ? b0 + k : count - 1);
        hipLaunchKernelGGL(stream_gather_kernel, dim3((unsigned)gx, (unsigned)nb, (unsigned)(1 + noise_rows)),
                           dim3(256), 0, (hipStream_t)stream, tab, b0, ring, (long long)cap, window,
                           (long long)noise_win, k0, k1, (unsigned long long)offset, mix, (long long)mix_bstride, nz,
                           (long long)nz_rstride, (long long)nz_bstride);
        const int lrc = ou_check_launch("stream_gather");
        if (lrc) return lrc;
    }
    return 0;
}

int ou_stream_overlap_add(const float* w, int64_t w_bstride, int window, int overlap, int64_t first, int count,
                          int closing, int64_t T, const float* fade, float* carry, float* out, int64_t* n_out,
                          void* stream)
{
    StreamGeom g;
    const int rc = stream_geom("stream_overlap_add", window, overlap, first, count, closing, T, &g);
    if (rc) return rc;
    const long long t_end = closing ? (long long)T : (first + count) * g.hop;
    const long long n = t_end - first * g.hop;
    if ((count > 0 && !w) || (n > 0 && !out)) return ou_fail(-1, "stream_overlap_add: null");
    if (overlap > 0 && (!fade || !carry))
        return ou_fail(-1, "stream_overlap_add: no fade table or no carry for overlap %d", overlap);
    if (count > 0 && w_bstride < window)
        return ou_fail(-1, "stream_overlap_add: count %d, stride %lld", count, (long long)w_bstride);
    if (((uintptr_t)w | (uintptr_t)carry | (uintptr_t)out) % 4)
        return ou_fail(-1, "stream_overlap_add: a buffer is not aligned to a float");
    if (n_out) *n_out = n;
    if (n == 0) return 0;   // closing from an empty carry (overlap 0): nothing is left to emit
    const long long gx = (n + 1023) / 1024;
    if (gx > kStreamMaxGrid) return ou_fail(-1, "stream_overlap_add: %lld samples are too many for one call", n);
    hipLaunchKernelGGL(stream_overlap_add_kernel, dim3((unsigned)gx), dim3(256), 0, (hipStream_t)stream, w,
                       (long long)w_bstride, g, fade, carry, out, t_end);
    return ou_check_launch("stream_overlap_add");
}

}  // extern "C"

#endif  // OU_STREAM_SHARED_ONLY
