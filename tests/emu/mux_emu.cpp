// The mux kernels (ou_mux.hip) on the CPU: the HIP source compiled for the host
// against tests/emu/hip/hip_runtime.h, under AddressSanitizer, every workgroup
// run (OUHIP_EMU_BLOCKS=0).  Every buffer is an exact-size heap block, so an
// access outside an array aborts with its location.  The kernels have no
// barriers and no LDS, and within one call no thread reads a word another
// stores, so the emulated values are real.  They are checked against a host
// restatement of the definition (include/ouhip.h, "Multiplexed streams"):
//   * the gather's MIX rows against the un-wrapped signal of the slot's
//     channel, over rings that wrap at different places, and its NZ rows
//     against a host loop over the same generator function (ou_normal.h) with
//     the slot's own (seed, offset), for window starts of every residue mod 4,
//     poison between the rows intact;
//   * the overlap-add inside whole mux sessions -- channels of different
//     lengths pushed at different paces, the slot rule restated here, padding
//     rows NaN, outputs and carries starting as NaN -- bit for bit per channel
//     against the per-sample rule of that channel's whole stream
//       own = min(t / H, n - 1);  y[t] = (0 + (1 - f) v_{own-1}) + f v_own
//     inside the owner's fade-in and 0 + 1 v_own elsewhere, each "+ w v" one
//     fused multiply-add as on the device; a closing run and a padding slot
//     must leave every carry as it was.
// Last, both entry points must refuse what the header says they refuse.
#include <cmath>

// the host has no sincospif; the emulated noise is compared with itself (the
// index mapping is under test here, the values are test_gpu_mux.py's)
inline void sincospif(float x, float* s, float* c)
{
    const double a = 3.14159265358979323846 * (double)x;
    *s = (float)std::sin(a);
    *c = (float)std::cos(a);
}

#ifndef OU_EMU_MUX_SRC
#define OU_EMU_MUX_SRC "../../open_universe_amd/csrc/ou_mux.hip"
#endif
#include OU_EMU_MUX_SRC

#include <algorithm>
#include <limits>
#include <random>
#include <set>
#include <vector>

namespace {

int g_launches = 0, g_refusals = 0;

#define OK(call)                                                                              \
    do {                                                                                      \
        const int rc_ = (call);                                                               \
        if (rc_ != 0) {                                                                       \
            std::fprintf(stderr, "%s:%d: %s returned %d: %s\n", __FILE__, __LINE__, #call, rc_, \
                         ouhip_detail::err_buf());                                            \
            std::exit(2);                                                                     \
        }                                                                                     \
        ++g_launches;                                                                         \
    } while (0)

#define REFUSED(call)                                                                         \
    do {                                                                                      \
        ouhip_detail::err_buf()[0] = 0;                                                       \
        if ((call) == 0) {                                                                    \
            std::fprintf(stderr, "%s:%d: %s was accepted\n", __FILE__, __LINE__, #call);      \
            std::exit(3);                                                                     \
        }                                                                                     \
        if (!ouhip_detail::err_buf()[0]) {                                                    \
            std::fprintf(stderr, "%s:%d: %s was refused without a text\n", __FILE__, __LINE__, #call); \
            std::exit(3);                                                                     \
        }                                                                                     \
        ++g_refusals;                                                                         \
    } while (0)

#define CHECK(cond, ...)                                                                      \
    do {                                                                                      \
        if (!(cond)) {                                                                        \
            std::fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond);                   \
            std::fprintf(stderr, __VA_ARGS__);                                                \
            std::fprintf(stderr, "\n");                                                       \
            std::exit(4);                                                                     \
        }                                                                                     \
    } while (0)

// an exact-size block of n floats starting `mis` floats past a 16-byte
// boundary: ASan guards both ends
struct Buf {
    char* raw;
    float* p;
    size_t n;
    Buf(size_t n_, int mis, float fill = 0.f) : n(n_)
    {
        raw = (char*)std::malloc((n + mis) * sizeof(float));
        p = (float*)raw + mis;
        for (size_t i = 0; i < n; ++i) p[i] = fill;
    }
    ~Buf() { std::free(raw); }
    Buf(const Buf&) = delete;
};

const float kPoison = 1e6f;
const float kNaN = std::numeric_limits<float>::quiet_NaN();

float signal(int c, long long p) { return (float)((p + 7919LL * c) % 65521) * 0.25f - 100.f * (c + 1); }

bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

// ---- gather ---------------------------------------------------------------
struct GChan {
    long long fed;
    uint64_t seed, offset;
};
struct GSlot {
    int c;
    long long start;
};

std::set<int> g_start_residues;

void run_gather(int W, long long cap, const std::vector<GChan>& ch, const std::vector<GSlot>& sl, int rows,
                long long win, long long gap, int mis_ring, int mis_y)
{
    const int C = (int)ch.size(), n = (int)sl.size();
    Buf rings((size_t)(C * cap), mis_ring, kPoison);
    for (int c = 0; c < C; ++c)
        for (long long p = std::max(0LL, ch[c].fed - cap); p < ch[c].fed; ++p) rings.p[c * cap + p % cap] = signal(c, p);
    const long long mbs = W + gap, nbs = win + gap, nrs = n * nbs + 5;
    Buf mix((size_t)((n - 1) * mbs + W), mis_y, kPoison);
    Buf nz(rows ? (size_t)((rows - 1) * nrs + (n - 1) * nbs + win) : 1, mis_y, kPoison);
    std::vector<ou_mux_slot> tab((size_t)n);
    for (int b = 0; b < n; ++b) {
        const GChan& s = ch[sl[b].c];
        tab[b] = {sl[b].start, std::max(0LL, s.fed - cap), s.fed, s.seed, s.offset, sl[b].c, 0};
        g_start_residues.insert((int)(sl[b].start & 3));
    }
    OK(ou_mux_gather(rings.p, cap, C, W, tab.data(), n, rows, win, mix.p, mbs, rows ? nz.p : nullptr, nrs, nbs, nullptr));
    std::vector<char> wm(mix.n, 0), wn(nz.n, 0);
    for (int b = 0; b < n; ++b) {
        const GChan& s = ch[sl[b].c];
        const long long st = sl[b].start;
        for (long long j = 0; j < W; ++j) {
            const size_t at = (size_t)(b * mbs + j);
            CHECK(same(mix.p[at], signal(sl[b].c, st + j)), "mix: slot %d (channel %d, start %lld) sample %lld: %g != %g",
                  b, sl[b].c, st, j, mix.p[at], signal(sl[b].c, st + j));
            wm[at] = 1;
        }
        const uint32_t k0 = (uint32_t)s.seed, k1 = (uint32_t)(s.seed >> 32);
        for (int r = 0; r < rows; ++r)
            for (long long j = 0; j < win; ++j) {
                const unsigned long long t = (unsigned long long)(st + j);
                float z[4];
                ouhip_detail::normal4(k0, k1, s.offset + ((unsigned long long)r << 38) + (t >> 2), z);
                const size_t at = (size_t)(r * nrs + b * nbs + j);
                CHECK(same(nz.p[at], z[t & 3]), "nz: row %d slot %d (channel %d, start %lld) sample %lld: %g != %g", r, b,
                      sl[b].c, st, j, nz.p[at], z[t & 3]);
                wn[at] = 1;
            }
    }
    for (size_t i = 0; i < mix.n; ++i) CHECK(wm[i] || mix.p[i] == kPoison, "mix[%zu] between the rows was written", i);
    if (rows)
        for (size_t i = 0; i < nz.n; ++i) CHECK(wn[i] || nz.p[i] == kPoison, "nz[%zu] between the rows was written", i);
}

void run_gathers()
{
    const int W = 64;
    for (int O : {0, 1, 7, 32}) {
        const long long H = W - O, cap = W + 3 * H;
        for (long long win : {64LL, 67LL})          // Tp - W = 0 and 3
            for (int mis = 0; mis < 4; ++mis) {
                // three channels whose rings wrap at different places (the last channel's too: its ring ends the
                // buffer): channel 0 has not wrapped yet, 1 and 2 wrap inside a window at places that are no
                // multiple of 4 apart; one channel is closing on a shifted last window; padding repeats a slot
                const long long f0 = cap - 1, f1 = cap + W / 2 + 1, f2 = 2 * cap + W / 2 + 3 + mis;
                std::vector<GChan> ch = {{f0, 7, 5}, {f1, 1ull << 40, ~0ull - 2}, {f2, 3, 1ull << 37}};
                std::vector<GSlot> sl = {{0, 0}, {0, H}, {1, (f1 - W) / H * H}, {1, f1 - W}, {2, (f2 - W) / H * H - H},
                                         {2, (f2 - W) / H * H}, {2, f2 - W}, {2, f2 - W}};
                run_gather(W, cap, ch, sl, 3, win, mis == 1 ? 36 : 0, mis, (mis + 1) % 4);
            }
        {   // a channel at window 0 beside one at positions past 2^32; no noise rows: MIX alone
            const long long far = (1LL << 32) + 5 * H + W + 3;
            std::vector<GChan> ch = {{W, 0, 0}, {far, 9, 9}};
            std::vector<GSlot> sl = {{0, 0}, {1, far - W - H}, {1, far - W}};
            run_gather(W, cap, ch, sl, 2, 67, 3, 1, 2);
            run_gather(W, cap, ch, sl, 0, 67, 8, 0, 0);
        }
        {   // a group of 33 slots: two launches; every channel two windows, then one padding slot
            const long long cap2 = W + 33 * H;
            std::vector<GChan> ch;
            std::vector<GSlot> sl;
            for (int c = 0; c < 16; ++c) {
                const long long fed = (c + 1) * H + W + (c % 4);
                ch.push_back({fed, (uint64_t)c * 11, (uint64_t)c << 20});
                sl.push_back({c, c * H});
                sl.push_back({c, (c + 1) * H});
            }
            sl.push_back(sl.back());
            run_gather(W, cap2, ch, sl, 2, 67, 0, 2, 3);
        }
    }
    CHECK(g_start_residues.size() == 4, "window starts of %zu residues mod 4", g_start_residues.size());
}

// ---- overlap-add inside whole sessions ------------------------------------------
std::vector<float> fade_table(int O)
{
    std::vector<float> f(2 * (size_t)O + 1);
    const double pi = 3.14159265358979323846;
    for (int u = 0; u < O; ++u) {
        const double s = std::sin(pi * (2.0 * u + 1.0) / (4.0 * O));
        f[u] = (float)(s * s);
        f[O + u] = (float)(1.0 - s * s);
    }
    return f;
}

struct Seen {
    bool two_in_group = false, across_groups = false, across_runs = false, window0 = false, padding = false;
    bool carry_only = false, only_carry_only = false, shifted = false, unshifted_close = false, t_w = false, t_w1 = false;
    bool two_launches = false, far = false;
    std::set<int> out_residues;
} seen;

// one channel of a session: a stream of T samples whose windows [i0, n) run in the session (i0 > 0: the session is
// joined at window i0, the carry holding the raw tail of window i0 - 1)
struct Chan {
    long long T, i0;
    long long n = 0, fed = 0, run = 0;
    int state = 1;                     // 1 open, 2 closing, 0 free
    std::vector<float> w;              // windows [max(i0 - 1, 0), n), W values each
    std::vector<float> want, got;      // samples [i0 H, T)
};

// Sessions of channels of the lengths Ts in a plan of batch B: every channel pushes pieces of `piece` samples (what
// its ring has room for), closes when all is in, and a run follows every round of pushes; with close_late a channel
// closes one round after its last push, so its regular windows have run by then.
void run_session(int W, int O, int B, std::vector<long long> Ts, std::vector<long long> i0s, std::vector<long long> piece,
                 bool close_late, int full_every, unsigned seed, int mis_out)
{
    const long long H = W - O, cap = W + (long long)B * H, bs = W + 3, cs = O + 2;
    const int C = (int)Ts.size();
    const std::vector<float> fade = fade_table(O);
    Buf tab((size_t)2 * O + (O ? 0 : 1), 0);
    for (int i = 0; i < 2 * O; ++i) tab.p[i] = fade[i];
    std::mt19937 gen(seed);
    std::uniform_real_distribution<float> dist(-1.f, 1.f);
    Buf carries((size_t)((C - 1) * cs + std::max(O, 1)), 1, kNaN);
    std::vector<Chan> ch((size_t)C);
    for (int c = 0; c < C; ++c) {
        Chan& s = ch[c];
        s.T = Ts[c], s.i0 = i0s[c];
        s.n = 1 + (s.T - W + H - 1) / H;
        const long long lo = std::max(s.i0 - 1, 0LL);
        s.w.resize((size_t)((s.n - lo) * W));
        for (float& v : s.w) v = dist(gen);
        auto row = [&](long long i) { return s.w.data() + (i - lo) * W; };
        auto start = [&](long long i) { return std::min(i * H, s.T - W); };
        for (long long t = s.i0 * H; t < s.T; ++t) {
            const long long own = std::min(t / H, s.n - 1), u = t - own * H;
            const float v = row(own)[t - start(own)];
            if (own > 0 && u < O)
                s.want.push_back(std::fma(fade[u], v, std::fma(fade[O + u], row(own - 1)[t - start(own - 1)], 0.f)));
            else
                s.want.push_back(std::fma(1.f, v, 0.f));
        }
        s.run = s.i0;
        s.fed = s.i0 ? (s.i0 - 1) * H + W : 0;     // what had been fed when window i0 - 1 ran
        if (s.i0)
            for (int u = 0; u < O; ++u) carries.p[c * cs + u] = row(s.i0 - 1)[H + u];
        if (s.i0 * H > (1LL << 32)) seen.far = true;
    }
    int round = 0;
    auto busy = [&] { return std::any_of(ch.begin(), ch.end(), [](const Chan& s) { return s.state != 0; }); };
    while (busy()) {
        CHECK(++round < 10000, "the session does not end");
        for (int c = 0; c < C; ++c) {
            Chan& s = ch[c];
            if (s.state != 1) continue;
            if (s.fed == s.T && (close_late || s.T == 0)) {
                s.state = 2;
                continue;
            }
            const long long retain = std::max(0LL, std::min(s.run * H, s.fed - W));
            const long long room = cap - (s.fed - retain);
            s.fed += std::min({piece[c], room, s.T - s.fed});
            if (s.fed == s.T && !close_late) s.state = 2;
        }
        // the slot rule
        struct Slot {
            int c;
            long long i;
        };
        std::vector<Slot> S;
        for (int c = 0; c < C; ++c) {
            const Chan& s = ch[c];
            if (s.state == 0) continue;
            const long long stop = s.state == 2 ? s.n : (s.fed < W ? 0 : (s.fed - W) / H + 1);
            for (long long i = s.run; i < stop; ++i) S.push_back({c, i});
        }
        const bool full = full_every && round % full_every == 0;
        if (full) S.resize(S.size() / B * B);
        // the runs, group by group; the carry-only closings go with the first group
        struct Group {
            std::vector<Slot> slots;
            std::vector<ou_mux_run> runs;
        };
        std::vector<Group> groups;
        for (size_t g = 0; g < S.size(); g += B) {
            Group G;
            G.slots.assign(S.begin() + g, S.begin() + std::min(S.size(), g + B));
            for (size_t b = 0; b < G.slots.size(); ++b) {
                const Slot& e = G.slots[b];
                if (!G.runs.empty() && G.runs.back().channel == e.c) {
                    ++G.runs.back().count;
                    seen.two_in_group = true;
                } else {
                    G.runs.push_back({e.i, 0, 0, 1, 0, (int32_t)b, e.c});
                }
            }
            groups.push_back(G);
        }
        std::vector<ou_mux_run> alone;
        for (int c = 0; c < C; ++c) {
            const Chan& s = ch[c];
            bool has = false;
            for (const Slot& e : S) has = has || e.c == c;
            if (s.state == 2 && s.run == s.n && !has) alone.push_back({s.n, s.T, 0, 0, 1, 0, c});
        }
        if (!alone.empty()) {
            seen.carry_only = true;
            if (groups.empty()) {
                groups.push_back({});
                seen.only_carry_only = true;
            }
            auto& r = groups[0].runs;
            r.insert(r.end(), alone.begin(), alone.end());
            std::sort(r.begin(), r.end(), [](const ou_mux_run& a, const ou_mux_run& b) { return a.channel < b.channel; });
        }
        // counts and offsets: channel-major in one buffer
        std::vector<long long> count((size_t)C, 0), at((size_t)C, 0);
        std::vector<long long> ran_to((size_t)C);
        for (int c = 0; c < C; ++c) ran_to[c] = ch[c].run;
        for (Group& G : groups)
            for (ou_mux_run& r : G.runs) {
                const Chan& s = ch[r.channel];
                if (s.state == 2 && r.first + r.count == s.n) r.closing = 1, r.T = s.T;
                count[r.channel] += (r.closing ? s.T : (r.first + r.count) * H) - r.first * H;
            }
        long long total = 0;
        for (int c = 0; c < C; ++c) at[c] = total, total += count[c];
        Buf out((size_t)total, mis_out, kNaN);
        std::vector<int> groups_of((size_t)C, 0);
        for (Group& G : groups) {
            const int ns = (int)G.slots.size();
            // OUT: the real slots' rows, the padding rows NaN -- they are computed by the plan and must not be read
            Buf w(ns ? (size_t)((B - 1) * bs + W) : 1, 2, kNaN);
            for (int b = 0; b < ns; ++b) {
                const Chan& s = ch[G.slots[b].c];
                std::memcpy(w.p + b * bs, s.w.data() + (G.slots[b].i - std::max(s.i0 - 1, 0LL)) * W, W * sizeof(float));
            }
            if (ns && ns < B) seen.padding = true;
            std::vector<float> before(carries.p, carries.p + carries.n);
            std::vector<int64_t> n_out(G.runs.size(), -1);
            for (ou_mux_run& r : G.runs) {
                r.out_off = at[r.channel];
                seen.out_residues.insert((int)(((uintptr_t)(out.p + r.out_off) >> 2) & 3));
                if (r.first == 0 && r.count) seen.window0 = true;
                if (r.count && groups_of[r.channel]++) seen.across_groups = true;
            }
            if (G.runs.size() > 32) seen.two_launches = true;
            OK(ou_mux_overlap_add(ns ? w.p : nullptr, bs, ns ? B : 0, W, O, G.runs.data(), (int)G.runs.size(),
                                  O ? tab.p : nullptr, O ? carries.p : nullptr, cs, C, total ? out.p : nullptr, total,
                                  n_out.data(), nullptr));
            for (size_t k = 0; k < G.runs.size(); ++k) {
                const ou_mux_run& r = G.runs[k];
                Chan& s = ch[r.channel];
                const long long n = (r.closing ? s.T : (r.first + r.count) * H) - r.first * H;
                CHECK(n_out[k] == n, "run %zu: %lld samples, expected %lld", k, (long long)n_out[k], n);
                at[r.channel] += n;
                ran_to[r.channel] = r.first + r.count;
                if (r.closing) {
                    const long long last = s.n - 1;
                    if (r.count && last * H > s.T - W) seen.shifted = true;
                    if (r.count && last * H == s.T - W) seen.unshifted_close = true;
                    if (s.T == W) seen.t_w = true;
                    if (s.T == W + 1) seen.t_w1 = true;
                }
                // the carry: a run that goes on leaves the raw tail of its last window, a closing run leaves it alone
                for (int u = 0; u < O; ++u) {
                    const float have = carries.p[r.channel * cs + u];
                    const float want = r.closing ? before[(size_t)(r.channel * cs + u)]
                                                 : w.p[(r.slot + r.count - 1) * bs + H + u];
                    CHECK(same(have, want), "channel %d carry[%d]: %g != %g", r.channel, u, have, want);
                }
            }
            // every word of the carries that belongs to no run of this group is as it was
            std::vector<char> touched(carries.n, 0);
            for (const ou_mux_run& r : G.runs)
                for (int u = 0; u < O; ++u) touched[(size_t)(r.channel * cs + u)] = 1;
            for (size_t i = 0; i < carries.n; ++i)
                CHECK(touched[i] || same(carries.p[i], before[i]), "carries[%zu] belongs to no run and was written", i);
        }
        // the run's buffer: channel c's samples at its offset, everything written exactly (NaN nowhere)
        long long off = 0;
        for (int c = 0; c < C; ++c) {
            Chan& s = ch[c];
            for (long long m = 0; m < count[c]; ++m) s.got.push_back(out.p[off + m]);
            off += count[c];
            CHECK(at[c] == off, "channel %d: its runs emitted up to %lld, its share ends at %lld", c, at[c], off);
            if (count[c] && s.run > s.i0 && ran_to[c] > s.run) seen.across_runs = true;
            s.run = ran_to[c];
            if (s.state == 2 && (long long)s.got.size() == s.T - s.i0 * H) s.state = 0;
        }
    }
    for (int c = 0; c < C; ++c) {
        const Chan& s = ch[c];
        CHECK(s.got.size() == s.want.size(), "channel %d: %zu samples, expected %zu", c, s.got.size(), s.want.size());
        for (size_t m = 0; m < s.want.size(); ++m)
            CHECK(same(s.got[m], s.want[m]), "W %d O %d B %d channel %d (T %lld) sample %lld: %.9g != %.9g", W, O, B, c,
                  s.T, (long long)(s.i0 * H + m), s.got[m], s.want[m]);
    }
}

void run_sessions()
{
    unsigned seed = 1;
    const int W = 64;
    for (int O : {0, 1, 7, 32}) {
        const long long H = W - O;
        for (int B : {1, 2, 3, 5}) {
            // T = W, T = W + 1 (a last window shifted by H - 1), T = W + 3 H (four regular windows: closes from the
            // carry alone when it closes late), a shifted last window after several groups
            std::vector<long long> Ts = {W, W + 1, W + 3 * H, W + 5 * H + H / 2 + 1};
            for (int late = 0; late < 2; ++late) {
                run_session(W, O, B, Ts, {0, 0, 0, 0}, {W / 2 + 1, 2 * W, H, 3 * H + 1}, late, 0, seed++, B % 4);
                run_session(W, O, B, Ts, {0, 0, 0, 0}, {1000, 1000, 1000, 1000}, late, 2, seed++, (B + 1) % 4);
            }
        }
        run_session(W, O, 2, {W + 3 * H}, {0}, {H}, true, 0, seed++, 0);   // its last run() is the carry alone
        // one channel joined at positions past 2^32 beside two ordinary ones
        const long long i0 = (1LL << 32) / H + 3;
        run_session(W, O, 2, {i0 * H + W + 2 * H + 5, W + 2 * H, W}, {i0, 0, 0}, {H, 2 * H, W}, true, 0, seed++, 3);
        run_session(W, O, 4, {i0 * H + W + 3 * H, W + 2 * H, W + 1}, {i0, 0, 0}, {3 * H, H, W}, true, 3, seed++, 1);
    }
    {   // 40 channels in one group of 40: 40 runs, two launches
        std::vector<long long> Ts, i0s, piece;
        for (int c = 0; c < 40; ++c) Ts.push_back(W + (c % 3) * (W - 7) + (c % 2)), i0s.push_back(0), piece.push_back(W);
        run_session(W, 7, 40, Ts, i0s, piece, false, 0, seed++, 2);
        run_session(W, 7, 40, Ts, i0s, piece, true, 0, seed++, 1);
    }
#define SEEN(what) CHECK(seen.what, "no session had: " #what)
    SEEN(two_in_group);
    SEEN(across_groups);
    SEEN(across_runs);
    SEEN(window0);
    SEEN(padding);
    SEEN(carry_only);
    SEEN(only_carry_only);
    SEEN(shifted);
    SEEN(unshifted_close);
    SEEN(t_w);
    SEEN(t_w1);
    SEEN(two_launches);
    SEEN(far);
    CHECK(seen.out_residues.size() == 4, "output offsets of %zu residues mod 4", seen.out_residues.size());
}

// ---- refusals -----------------------------------------------------------------
void run_rejections()
{
    Buf rings(64, 0), m(64, 0), z(64, 0), f(8, 0), c(16, 0), y(64, 0);
    // W 8, O 2: H 6; two rings of 20; channel 0 holds [0, 20), channel 1 [5, 25)
    const ou_mux_slot good[3] = {{0, 0, 20, 1, 0, 0, 0}, {12, 0, 20, 1, 0, 0, 0}, {17, 5, 25, 2, 9, 1, 0}};
#define GATHER(rings_, cap, C, W, slots_, n, rows, win, mix, mbs, nz, nrs, nbs) \
    ou_mux_gather(rings_, cap, C, W, slots_, n, rows, win, mix, mbs, nz, nrs, nbs, nullptr)
    OK(GATHER(rings.p, 20, 2, 8, good, 3, 2, 9, m.p, 8, z.p, 27, 9));
    OK(GATHER(rings.p, 20, 2, 8, good, 2, 0, 0, m.p, 8, nullptr, 0, 0));      // no noise rows: no NZ
    REFUSED(GATHER(nullptr, 20, 2, 8, good, 3, 2, 9, m.p, 8, z.p, 27, 9));
    REFUSED(GATHER(rings.p, 20, 2, 8, nullptr, 3, 2, 9, m.p, 8, z.p, 27, 9));
    REFUSED(GATHER(rings.p, 20, 2, 8, good, 3, 2, 9, nullptr, 8, z.p, 27, 9));
    REFUSED(GATHER(rings.p, 20, 2, 8, good, 3, 2, 9, m.p, 8, nullptr, 27, 9));
    REFUSED(GATHER(rings.p, 20, 2, 0, good, 3, 2, 9, m.p, 8, z.p, 27, 9));     // W
    REFUSED(GATHER(rings.p, 7, 2, 8, good, 3, 2, 9, m.p, 8, z.p, 27, 9));      // cap < W
    REFUSED(GATHER(rings.p, 20, 0, 8, good, 3, 2, 9, m.p, 8, z.p, 27, 9));     // no channels
    REFUSED(GATHER(rings.p, 20, 1, 8, good, 3, 2, 9, m.p, 8, z.p, 27, 9));     // slot 2 names channel 1 of 1
    REFUSED(GATHER(rings.p, 20, 2, 8, good, 0, 2, 9, m.p, 8, z.p, 27, 9));     // no slots
    REFUSED(GATHER(rings.p, 20, 2, 8, good, 3, -1, 9, m.p, 8, z.p, 27, 9));    // rows
    REFUSED(GATHER(rings.p, 20, 2, 8, good, 3, 2, 0, m.p, 8, z.p, 27, 9));     // noise_win
    REFUSED(GATHER(rings.p, 20, 2, 8, good, 3, 2, 9, m.p, 7, z.p, 27, 9));     // MIX rows overlap
    REFUSED(GATHER(rings.p, 20, 2, 8, good, 3, 2, 9, m.p, 8, z.p, 27, 8));     // NZ items overlap
    REFUSED(GATHER(rings.p, 20, 2, 8, good, 3, 2, 9, m.p, 8, z.p, 26, 9));     // NZ rows overlap
    auto one = [&](ou_mux_slot s, long long win = 9) { return GATHER(rings.p, 20, 2, 8, &s, 1, 2, win, m.p, 8, z.p, 27, 9); };
    OK(one({12, 0, 20, 1, 0, 0, 0}));
    REFUSED(one({12, 0, 20, 1, 0, -1, 0}));      // channel
    REFUSED(one({12, 0, 20, 1, 0, 2, 0}));
    REFUSED(one({12, -1, 19, 1, 0, 0, 0}));      // lo
    REFUSED(one({12, 0, 21, 1, 0, 0, 0}));       // fed - lo > cap
    REFUSED(one({12, 21, 20, 1, 0, 0, 0}));      // fed < lo
    REFUSED(one({13, 0, 20, 1, 0, 0, 0}));       // the window ends past fed
    REFUSED(one({4, 5, 25, 1, 0, 0, 0}));        // the window starts below lo
    REFUSED(one({-1, 0, 20, 1, 0, 0, 0}));
    REFUSED(one({0, 0, 7, 1, 0, 0, 0}));         // fewer samples than one window
    {   // noise past sample 2^40
        const long long fed = 1LL << 40;
        REFUSED(one({fed - 8, fed - 20, fed, 1, 0, 1, 0}));
        OK(one({fed - 8, fed - 20, fed, 1, 0, 1, 0}, 8));
        REFUSED(one({fed - 7, fed - 19, fed + 1, 1, 0, 1, 0}, 1));   // fed itself past 2^40
    }

    // W 8, O 2, H 6; OUT holds 4 slots; channel 0 runs windows 0, 1; channel 1 window 3 (its carry is there)
    const ou_mux_run ok2[2] = {{0, 0, 0, 2, 0, 0, 0}, {3, 0, 12, 1, 0, 2, 1}};
#define OADD(w, wbs, ns, W, O, runs_, nr, fade, carries_, cs, C, out, len) \
    ou_mux_overlap_add(w, wbs, ns, W, O, runs_, nr, fade, carries_, cs, C, out, len, nullptr, nullptr)
    OK(OADD(m.p, 8, 4, 8, 2, ok2, 2, f.p, c.p, 2, 2, y.p, 18));
    OK(OADD(m.p, 8, 4, 8, 0, ok2, 1, nullptr, nullptr, 0, 2, y.p, 16));          // O = 0 needs neither table nor carries
    REFUSED(OADD(nullptr, 8, 4, 8, 2, ok2, 2, f.p, c.p, 2, 2, y.p, 18));
    REFUSED(OADD(m.p, 8, 4, 8, 2, nullptr, 2, f.p, c.p, 2, 2, y.p, 18));
    REFUSED(OADD(m.p, 8, 4, 8, 2, ok2, 0, f.p, c.p, 2, 2, y.p, 18));              // no runs
    REFUSED(OADD(m.p, 8, 4, 8, 2, ok2, 2, f.p, c.p, 2, 2, nullptr, 18));
    REFUSED(OADD(m.p, 8, 4, 8, 2, ok2, 2, nullptr, c.p, 2, 2, y.p, 18));          // O > 0 needs the table
    REFUSED(OADD(m.p, 8, 4, 8, 2, ok2, 2, f.p, nullptr, 2, 2, y.p, 18));          // and the carries
    REFUSED(OADD(m.p, 8, 4, 8, 2, ok2, 2, f.p, c.p, 1, 2, y.p, 18));              // carries overlap
    REFUSED(OADD(m.p, 8, 4, 0, 0, ok2, 2, f.p, c.p, 2, 2, y.p, 18));              // W
    REFUSED(OADD(m.p, 8, 4, 8, 5, ok2, 2, f.p, c.p, 5, 2, y.p, 18));              // O > W / 2
    REFUSED(OADD(m.p, 8, 4, 8, -1, ok2, 2, f.p, c.p, 2, 2, y.p, 18));
    REFUSED(OADD(m.p, 7, 4, 8, 2, ok2, 2, f.p, c.p, 2, 2, y.p, 18));              // windows overlap in w
    REFUSED(OADD(m.p, 8, 2, 8, 2, ok2, 2, f.p, c.p, 2, 2, y.p, 18));              // run 1's slot is past OUT
    REFUSED(OADD(m.p, 8, 4, 8, 2, ok2, 2, f.p, c.p, 2, 1, y.p, 18));              // channel 1 of 1
    REFUSED(OADD(m.p, 8, 4, 8, 2, ok2, 2, f.p, c.p, 2, 2, y.p, 17));              // run 1 writes past out
    auto two = [&](ou_mux_run a, ou_mux_run b) {
        const ou_mux_run r[2] = {a, b};
        return OADD(m.p, 8, 4, 8, 2, r, 2, f.p, c.p, 2, 2, y.p, 40);
    };
    OK(two({0, 0, 0, 2, 0, 0, 0}, {3, 0, 12, 1, 0, 2, 1}));
    OK(two({3, 20, 0, 0, 1, 0, 0}, {0, 20, 2, 3, 1, 0, 1}));                      // a carry-only closing and a closing run
    REFUSED(two({0, 0, 0, 2, 0, 0, 0}, {3, 0, 12, 1, 0, 2, 0}));                  // two runs of one channel
    REFUSED(two({0, 0, 0, 2, 0, 0, 1}, {3, 0, 12, 1, 0, 2, 0}));                  // channels descend
    REFUSED(two({0, 0, 0, 2, 0, 0, 0}, {3, 0, 12, 1, 0, 1, 1}));                  // slots overlap
    REFUSED(two({0, 0, 0, 2, 0, -1, 0}, {3, 0, 12, 1, 0, 2, 1}));
    REFUSED(two({0, 0, 0, 2, 0, 0, 0}, {3, 0, 11, 1, 0, 2, 1}));                  // outputs overlap
    REFUSED(two({0, 0, -1, 2, 0, 0, 0}, {3, 0, 12, 1, 0, 2, 1}));
    REFUSED(two({-1, 0, 0, 2, 0, 0, 0}, {3, 0, 12, 1, 0, 2, 1}));                 // first
    REFUSED(two({0, 0, 0, 0, 0, 0, 0}, {3, 0, 12, 1, 0, 2, 1}));                  // count < 1 and not closing
    REFUSED(two({0, 0, 0, -1, 1, 0, 0}, {3, 0, 12, 1, 0, 2, 1}));
    REFUSED(two({0, 7, 0, 1, 1, 0, 0}, {3, 0, 12, 1, 0, 2, 1}));                  // closing: T < W
    REFUSED(two({0, 20, 0, 2, 1, 0, 0}, {3, 0, 12, 1, 0, 2, 1}));                 // closing: T has 3 windows
    REFUSED(two({3, 19, 0, 0, 1, 0, 0}, {3, 0, 12, 1, 0, 2, 1}));                 // closing without windows: window 2 shifted
}

}  // namespace

int main()
{
    run_gathers();
    run_sessions();
    run_rejections();
    std::printf("ok: %d launches checked, %d calls refused\n", g_launches, g_refusals);
    return 0;
}
