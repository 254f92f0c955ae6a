// ou_mux.hip -- the two kernels around multiplexed streams (include/ouhip.h,
// "Multiplexed streams"): several section-15 streams, each
// with its own ring, carry and noise, whose ready windows share the slots of one
// batched plan.
//
//  * ou_mux_gather       fills every slot's MIX row from its channel's ring and
//                        generates all NZ rows in place, one launch per group
//  * ou_mux_overlap_add  emits, per channel, the samples the group makes final,
//                        one launch per group
//
// Per slot and per channel they give the bits of ou_stream_gather and
// ou_stream_overlap_add called for that channel alone: the noise is the shared
// generator (ou_normal.h), the per-sample rule of the overlap-add the shared
// stream_emit_quad (ou_stream.hip).  The entry points keep no state and allocate
// nothing; every argument is checked on the host.  A launch gets its slots or
// runs as a by-value table of at most kMuxEntries entries; a larger call is
// several launches.  Sample positions are 64-bit; every store is a plain vector
// store.
#define OU_STREAM_SHARED_ONLY
#include "ou_stream.hip"
#undef OU_STREAM_SHARED_ONLY

namespace {

constexpr int kMuxEntries = 32;   // slots or runs per launch: the tables below travel as kernel arguments

struct MuxSlot {
    long long s;                  // start of the window in its channel's stream
    unsigned long long offset;
    uint32_t k0, k1;
    int channel, pad;
};
struct MuxSlotTable {
    MuxSlot e[kMuxEntries];
};

struct MuxRun {
    long long first, T, t_end, out_off;
    int count, closing, slot, channel;
};
struct MuxRunTable {
    MuxRun e[kMuxEntries];
};

// grid (lanes / 256, slots of the launch, 1 + noise_rows): stream_gather_kernel
// with the ring, the start and the key of the noise read per slot.
// z = 0 copies the slot's window of its channel's ring to MIX, four samples per
// lane; the ring holds position p at p mod cap, so a lane's four may wrap.
// z = 1 + r generates noise row r: a lane owns counter q = (s >> 2) + lane of
// the channel's draw, whose four normals land at j0 = 4 q - s in the row,
// -4 < j0; the first and the last lane of a row may hold fewer than four of its
// values and take the guarded dword path.
__global__ void __launch_bounds__(256) mux_gather_kernel(MuxSlotTable tab, int b0, const float* __restrict__ rings,
                                                         long long cap, int W, long long noise_win,
                                                         float* __restrict__ mix, long long mix_bstride,
                                                         float* __restrict__ nz, long long nz_rstride,
                                                         long long nz_bstride)
{
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    const MuxSlot& e = tab.e[blockIdx.y];
    const long long s = e.s;
    const long long b = (long long)b0 + blockIdx.y;
    if (blockIdx.z == 0) {
        const long long j = lane * 4;
        if (j >= W) return;
        const float* ring = rings + (long long)e.channel * cap;
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
    ouhip_detail::normal4(e.k0, e.k1, e.offset + ((unsigned long long)r << 38) + (unsigned long long)q, z);
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

// grid (sample quads / 256, runs of the launch).  Run y is one channel's
// ou_stream_overlap_add: its slots start at w + slot w_bstride, its carry is
// the channel's, its samples go to out + out_off.  Runs share neither slots,
// nor a carry, nor a word of out (checked on the host), so what
// stream_emit_quad promises within one stream holds across the launch.  Slots
// of no run are never addressed.
__global__ void __launch_bounds__(256) mux_overlap_add_kernel(MuxRunTable tab, const float* __restrict__ w,
                                                              long long w_bstride, int W, int O,
                                                              const float* __restrict__ fade,
                                                              float* __restrict__ carries, long long carry_stride,
                                                              float* __restrict__ out)
{
    const MuxRun& e = tab.e[blockIdx.y];
    StreamGeom g;
    g.hop = W - O, g.first = e.first, g.T = e.T;
    g.W = W, g.O = O, g.count = e.count, g.closing = e.closing;
    stream_emit_quad(w + (long long)e.slot * w_bstride, w_bstride, g, fade,
                     carries ? carries + (long long)e.channel * carry_stride : nullptr, out + e.out_off, e.t_end,
                     ((long long)blockIdx.x * 256 + threadIdx.x) * 4);
}

}  // namespace

extern "C" {

int ou_mux_gather(const float* rings, int64_t cap, int channels, int window, const ou_mux_slot* slots, int n_slots,
                  int noise_rows, int64_t noise_win, float* mix, int64_t mix_bstride, float* nz, int64_t nz_rstride,
                  int64_t nz_bstride, void* stream)
{
    if (!rings || !slots || !mix || (noise_rows > 0 && !nz)) return ou_fail(-1, "mux_gather: null");
    if (window <= 0 || cap < window || channels < 1)
        return ou_fail(-1, "mux_gather: window %d, %d rings of %lld samples", window, channels, (long long)cap);
    if (n_slots < 1 || n_slots > 65535 || noise_rows < 0 || noise_rows > 65534 || (noise_rows > 0 && noise_win < 1))
        return ou_fail(-1, "mux_gather: %d slots, noise rows %d, noise window %lld", n_slots, noise_rows,
                       (long long)noise_win);
    if (((uintptr_t)rings | (uintptr_t)mix | (uintptr_t)nz) % 4)
        return ou_fail(-1, "mux_gather: a buffer is not aligned to a float");
    if (mix_bstride < window || (noise_rows > 0 && (nz_bstride < noise_win ||
                                                    nz_rstride < (long long)(n_slots - 1) * nz_bstride + noise_win)))
        return ou_fail(-1, "mux_gather: rows or items overlap (strides %lld, %lld, %lld)", (long long)mix_bstride,
                       (long long)nz_rstride, (long long)nz_bstride);
    for (int b = 0; b < n_slots; ++b) {
        const ou_mux_slot& s = slots[b];
        if (s.channel < 0 || s.channel >= channels)
            return ou_fail(-1, "mux_gather: slot %d names channel %d of %d", b, s.channel, channels);
        if (s.lo < 0 || s.fed < s.lo || s.fed - s.lo > cap || s.fed > kStreamMaxSamples)
            return ou_fail(-1, "mux_gather: slot %d: a ring of %lld samples holding [%lld, %lld)", b, (long long)cap,
                           (long long)s.lo, (long long)s.fed);
        if (s.start < s.lo || s.start > s.fed - window)
            return ou_fail(-1, "mux_gather: slot %d covers [%lld, %lld), channel %d's ring holds [%lld, %lld)", b,
                           (long long)s.start, (long long)s.start + window, s.channel, (long long)s.lo,
                           (long long)s.fed);
        if (noise_rows > 0 && s.start + noise_win > kStreamMaxSamples)
            return ou_fail(-1, "mux_gather: slot %d draws noise past sample 2^40", b);
    }
    const long long wl = ((long long)window + 3) / 4;
    const long long nl = noise_rows > 0 ? ((long long)noise_win + 3) / 4 + 1 : 0;   // counters a row can touch
    const long long gx = ((wl > nl ? wl : nl) + 255) / 256;
    if (gx > kStreamMaxGrid) return ou_fail(-1, "mux_gather: window %lld is too long", (long long)noise_win);
    for (int b0 = 0; b0 < n_slots; b0 += kMuxEntries) {
        const int nb = n_slots - b0 < kMuxEntries ? n_slots - b0 : kMuxEntries;
        MuxSlotTable tab = {};
        for (int k = 0; k < nb; ++k) {
            const ou_mux_slot& s = slots[b0 + k];
            tab.e[k].s = s.start;
            tab.e[k].offset = s.offset;
            tab.e[k].k0 = (uint32_t)s.seed, tab.e[k].k1 = (uint32_t)(s.seed >> 32);
            tab.e[k].channel = s.channel;
        }
        hipLaunchKernelGGL(mux_gather_kernel, dim3((unsigned)gx, (unsigned)nb, (unsigned)(1 + noise_rows)), dim3(256),
                           0, (hipStream_t)stream, tab, b0, rings, (long long)cap, window, (long long)noise_win, mix,
                           (long long)mix_bstride, nz, (long long)nz_rstride, (long long)nz_bstride);
        const int lrc = ou_check_launch("mux_gather");
        if (lrc) return lrc;
    }
    return 0;
}

int ou_mux_overlap_add(const float* w, int64_t w_bstride, int n_slots, int window, int overlap,
                       const ou_mux_run* runs, int n_runs, const float* fade, float* carries, int64_t carry_stride,
                       int channels, float* out, int64_t out_len, int64_t* n_out, void* stream)
{
    if (!runs || n_runs < 1 || n_runs > 65535 || n_slots < 0 || channels < 1 || out_len < 0)
        return ou_fail(-1, "mux_overlap_add: %d runs over %d slots, %d channels, %lld samples of output", n_runs,
                       n_slots, channels, (long long)out_len);
    if (overlap > 0 && (!fade || !carries))
        return ou_fail(-1, "mux_overlap_add: no fade table or no carries for overlap %d", overlap);
    if (carries && carry_stride < overlap)
        return ou_fail(-1, "mux_overlap_add: carries %lld apart hold %d samples each", (long long)carry_stride,
                       overlap);
    if (((uintptr_t)w | (uintptr_t)carries | (uintptr_t)out) % 4)
        return ou_fail(-1, "mux_overlap_add: a buffer is not aligned to a float");
    // pass 1: every run is checked before anything is launched
    int next_slot = 0, last_channel = -1;
    long long next_out = 0, most = 0;
    for (int r = 0; r < n_runs; ++r) {
        const ou_mux_run& u = runs[r];
        StreamGeom g;
        const int rc = stream_geom("mux_overlap_add", window, overlap, u.first, u.count, u.closing, u.T, &g);
        if (rc) return rc;
        if (u.channel <= last_channel || u.channel >= channels)
            return ou_fail(-1, "mux_overlap_add: run %d is channel %d after channel %d, of %d", r, u.channel,
                           last_channel, channels);
        if (u.count > 0 && (u.slot < next_slot || u.slot > n_slots - u.count))
            return ou_fail(-1, "mux_overlap_add: run %d has the slots [%d, %d) of %d, the run before ends at %d", r,
                           u.slot, u.slot + u.count, n_slots, next_slot);
        const long long n = (u.closing ? (long long)u.T : (u.first + u.count) * g.hop) - u.first * g.hop;
        if (u.out_off < next_out || u.out_off > out_len - n)
            return ou_fail(-1, "mux_overlap_add: run %d writes [%lld, %lld) of %lld, the run before ends at %lld", r,
                           (long long)u.out_off, (long long)u.out_off + n, (long long)out_len, next_out);
        if (u.count > 0) next_slot = u.slot + u.count;
        last_channel = u.channel;
        next_out = u.out_off + n;
        if (n > most) most = n;
    }
    if (next_slot > 0 && (!w || w_bstride < window))
        return ou_fail(-1, "mux_overlap_add: %s, stride %lld", w ? "windows overlap in w" : "null", (long long)w_bstride);
    if (most > 0 && !out) return ou_fail(-1, "mux_overlap_add: null");
    if (n_out)
        for (int r = 0; r < n_runs; ++r)
            n_out[r] = (runs[r].closing ? (long long)runs[r].T : (runs[r].first + runs[r].count) * (window - overlap)) -
                       runs[r].first * (window - overlap);
    if (most == 0) return 0;   // closings from empty carries (overlap 0): nothing is left to emit
    if ((most + 1023) / 1024 > kStreamMaxGrid)
        return ou_fail(-1, "mux_overlap_add: %lld samples are too many for one call", most);
    for (int r0 = 0; r0 < n_runs; r0 += kMuxEntries) {
        const int nr = n_runs - r0 < kMuxEntries ? n_runs - r0 : kMuxEntries;
        MuxRunTable tab = {};
        long long big = 0;
        for (int k = 0; k < nr; ++k) {
            const ou_mux_run& u = runs[r0 + k];
            const long long hop = window - overlap;
            MuxRun& e = tab.e[k];
            e.first = u.first, e.T = u.closing ? u.T : 0;
            e.t_end = u.closing ? (long long)u.T : (u.first + u.count) * hop;
            e.out_off = u.out_off;
            e.count = u.count, e.closing = u.closing ? 1 : 0, e.slot = u.count > 0 ? u.slot : 0, e.channel = u.channel;
            const long long n = e.t_end - u.first * hop;
            if (n > big) big = n;
        }
        if (big == 0) continue;
        hipLaunchKernelGGL(mux_overlap_add_kernel, dim3((unsigned)((big + 1023) / 1024), (unsigned)nr), dim3(256), 0,
                           (hipStream_t)stream, tab, w, (long long)w_bstride, window, overlap, fade, carries,
                           (long long)carry_stride, out);
        const int lrc = ou_check_launch("mux_overlap_add");
        if (lrc) return lrc;
    }
    return 0;
}

}  // extern "C"
