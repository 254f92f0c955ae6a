// The streaming kernels (ou_stream.hip) on the CPU: the HIP source compiled for
// the host against tests/emu/hip/hip_runtime.h, under AddressSanitizer, every
// workgroup run (OUHIP_EMU_BLOCKS=0).  Every buffer is an exact-size heap block,
// so an access outside an array aborts with its location.  The kernels have no
// barriers and no LDS, and within one call no thread reads a word another
// stores, so the emulated values are real.  They are checked against a host
// restatement of the definition (include/ouhip.h, "Streaming enhance"):
//   * the gather's MIX rows against the un-wrapped signal, over a ring that
//     wraps, and its NZ rows against a host loop over the same generator
//     function (ou_normal.h) -- sample t of draw k is lane t & 3 of counter
//     offset + k 2^38 + (t >> 2) -- for window starts of every residue mod 4,
//     poison between the rows intact;
//   * the overlap-add, from outputs and a carry that start as NaN, bit for bit
//     against the per-sample rule of the whole stream
//       own = min(t / H, n - 1);  y[t] = (0 + (1 - f) v_{own-1}) + f v_own
//     inside the owner's fade-in and 0 + 1 v_own elsewhere, each "+ w v" one
//     fused multiply-add as on the device, for every grouping and every way a
//     stream can close.
// Last, both entry points must refuse what the header says they refuse.
#include <cmath>

// the host has no sincospif; the emulated noise is compared with itself (the
// index mapping is under test here, the values are test_gpu_stream.py's)
inline void sincospif(float x, float* s, float* c)
{
    const double a = 3.14159265358979323846 * (double)x;
    *s = (float)std::sin(a);
    *c = (float)std::cos(a);
}

#include "../../open_universe_amd/csrc/ou_stream.hip"

#include <limits>
#include <random>
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

float signal(long long p) { return (float)(p % 65521) * 0.25f - 100.f; }

bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

// ---- gather ---------------------------------------------------------------
// windows [first, first + count) of a stream with `fed` samples in a ring of
// `cap`; closing: T = fed
void run_gather(int W, int O, long long cap, long long fed, long long first, int count, int slots, int closing,
                int rows, long long win, long long gap, int mis_ring, int mis_y, uint64_t seed, uint64_t offset)
{
    const long long H = W - O, lo = fed > cap ? fed - cap : 0;
    Buf ring((size_t)cap, mis_ring, kPoison);
    for (long long p = lo; p < fed; ++p) ring.p[p % cap] = signal(p);
    const long long mbs = W + gap, nbs = win + gap, nrs = slots * nbs + 5;
    Buf mix((size_t)((slots - 1) * mbs + W), mis_y, kPoison);
    Buf nz(rows ? (size_t)((rows - 1) * nrs + (slots - 1) * nbs + win) : 1, mis_y, kPoison);
    OK(ou_stream_gather(ring.p, cap, lo, fed, W, O, first, count, slots, closing, closing ? fed : 0, rows, win, seed,
                        offset, mix.p, mbs, rows ? nz.p : nullptr, nrs, nbs, nullptr));
    std::vector<char> wm(mix.n, 0), wn(nz.n, 0);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int b = 0; b < slots; ++b) {
        const long long i = first + (b < count ? b : count - 1);
        long long s = i * H;
        if (closing && i == first + count - 1 && s > fed - W) s = fed - W;
        for (long long j = 0; j < W; ++j) {
            const size_t at = (size_t)(b * mbs + j);
            CHECK(same(mix.p[at], signal(s + j)), "mix: slot %d sample %lld: %g != %g", b, j, mix.p[at], signal(s + j));
            wm[at] = 1;
        }
        for (int r = 0; r < rows; ++r)
            for (long long j = 0; j < win; ++j) {
                const unsigned long long t = (unsigned long long)(s + j);
                float z[4];
                ouhip_detail::normal4(k0, k1, offset + ((unsigned long long)r << 38) + (t >> 2), z);
                const size_t at = (size_t)(r * nrs + b * nbs + j);
                CHECK(same(nz.p[at], z[t & 3]), "nz: row %d slot %d (start %lld) sample %lld: %g != %g", r, b, s, j,
                      nz.p[at], z[t & 3]);
                wn[at] = 1;
            }
    }
    for (size_t i = 0; i < mix.n; ++i) CHECK(wm[i] || mix.p[i] == kPoison, "mix[%zu] between the rows was written", i);
    if (rows)
        for (size_t i = 0; i < nz.n; ++i) CHECK(wn[i] || nz.p[i] == kPoison, "nz[%zu] between the rows was written", i);
}

void run_gathers()
{
    // the ragged last counter where the row ends with the block at a 16-byte aligned base: an unguarded 16-byte
    // store leaves it
    run_gather(4000, 800, 7200, 4000, 0, 1, 1, 0, 1, 4163, 0, 0, 0, 1, 0);
    for (long long win : {4160LL, 4163LL})
        for (int mis = 0; mis < 4; ++mis) {
            // O = 801: H = 3199, the starts 0, 3199, 6398, 9597 have the residues 0, 3, 2, 1 mod 4
            run_gather(4000, 801, 4000 + 2 * 3199, 13597, 2, 2, 2, 0, 3, win, 0, mis, 0, 7, 5);          // wraps
            run_gather(4000, 801, 4000 + 2 * 3199, 7199, 0, 2, 2, 0, 3, win, 36, 0, mis, 7, 5);          // no wrap yet
            run_gather(4000, 801, 4000 + 3 * 3199, 13600, 1, 3, 3, 0, 2, win, 1, mis, mis, 1ull << 40, ~0ull - 2);
            // closing: the last window shifted back to T - W, T - W of every residue; the unused slot repeats it
            run_gather(4000, 800, 4000 + 3 * 3200, 9001 + mis, 1, 2, 3, 1, 3, win, 0, mis, 1, 3, 1ull << 37);
        }
    run_gather(4000, 800, 7200, 4000, 0, 1, 2, 1, 3, 4160, 0, 0, 0, 0, 0);    // T = W: one window and its copy
    run_gather(4000, 0, 8000, 12000, 1, 2, 2, 0, 0, 4160, 8, 1, 0, 0, 0);     // no noise rows: MIX alone
    // W % 4 != 0, a ring barely larger than the window, many slots (two launches), a stream past 2^32 samples
    run_gather(37, 5, 37 + 40 * 32, 40 * 32 + 37, 0, 40, 40, 0, 2, 41, 0, 1, 2, 9, 9);
    run_gather(37, 5, 101, (1LL << 32) + 3 * 32 + 37, (1LL << 27) + 1, 2, 2, 0, 2, 41, 3, 3, 1, 9, 9);
    run_gather(37, 5, 101, (1LL << 32) + 3 * 32 + 38, (1LL << 27) + 3, 2, 3, 1, 2, 64, 0, 0, 3, 9, 9);
}

// ---- overlap-add ------------------------------------------------------------
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

// a stream of T samples in groups of B: the calls a session makes, whatever the cuts of the pushes were
void run_overlap_add(long long T, int W, int O, std::vector<int> Bs, unsigned seed, int mis_out)
{
    const long long H = W - O, n = 1 + (T - W + H - 1) / H, bs = W + 8;
    std::vector<long long> st;
    for (long long i = 0; i < n; ++i) st.push_back(std::min(i * H, T - W));
    Buf w((size_t)((n - 1) * bs + W), 1);
    std::mt19937 gen(seed);
    std::uniform_real_distribution<float> dist(-1.f, 1.f);
    for (size_t i = 0; i < w.n; ++i) w.p[i] = dist(gen);
    const std::vector<float> fade = fade_table(O);
    Buf tab((size_t)2 * O + (O ? 0 : 1), 0);
    for (int i = 0; i < 2 * O; ++i) tab.p[i] = fade[i];
    const float* ft = O ? tab.p : nullptr;

    std::vector<float> want;   // the per-sample rule over the whole stream
    for (long long t = 0; t < T; ++t) {
        const long long own = std::min(t / H, n - 1), u = t - own * H;
        const float v = w.p[own * bs + (t - st[own])];
        if (own > 0 && u < O) {
            const float vp = w.p[(own - 1) * bs + (t - st[own - 1])];
            want.push_back(std::fma(fade[u], v, std::fma(fade[O + u], vp, 0.f)));
        } else {
            want.push_back(std::fma(1.f, v, 0.f));
        }
    }

    for (int B : Bs) {
        Buf y((size_t)T, mis_out, kNaN);
        Buf carry((size_t)(O ? O : 1), 0, kNaN);
        float* cp = O ? carry.p : nullptr;
        const long long ready = (T - W) / H + 1;   // regular windows whose samples all arrive before close
        const long long run = ready / B * B;
        long long total = 0;
        int64_t got = -1;
        for (long long first = 0; first < run; first += B) {
            OK(ou_stream_overlap_add(w.p + first * bs, bs, W, O, first, B, 0, 0, ft, cp, y.p + first * H, &got, nullptr));
            CHECK(got == B * H, "T %lld B %d first %lld: emitted %lld", T, B, first, (long long)got);
            total += got;
        }
        // close: the windows that are left, or the carry alone
        OK(ou_stream_overlap_add(n > run ? w.p + run * bs : nullptr, bs, W, O, run, (int)(n - run), 1, T, ft, cp,
                                 y.p + run * H, &got, nullptr));
        CHECK(total + got == T, "T %lld B %d: emitted %lld in all", T, B, (long long)(total + got));
        for (long long t = 0; t < T; ++t)
            CHECK(same(y.p[t], want[(size_t)t]), "T %lld W %d O %d B %d sample %lld: %.9g != %.9g", T, W, O, B, t,
                  y.p[t], want[(size_t)t]);
    }
}

void run_overlap_adds()
{
    unsigned seed = 1;
    for (int O : {800, 801, 0, 2000})
        for (long long T : {4000LL, 4001LL, 9000LL, 9001LL, 10400LL, 13600LL})
            run_overlap_add(T, 4000, O, {1, 2, 3, 5}, seed++, (int)(T % 4));
    // T = W + 3 H: four regular windows, so B = 1, 2, 4 close from the carry alone and B = 3 with one window left
    for (int O : {18, 5, 0}) {
        run_overlap_add(37 + 3 * (37 - O), 37, O, {1, 2, 3, 4, 5}, seed++, 1);
        run_overlap_add(37 + 3 * (37 - O) + 1, 37, O, {1, 2, 3, 4, 5}, seed++, 2);   // a last window shifted by H - 1
        run_overlap_add(37, 37, O, {1, 2}, seed++, 3);                               // T = W
        run_overlap_add(38, 37, O, {1, 2, 3}, seed++, 0);                            // T = W + 1
        run_overlap_add(2000, 37, O, {1, 7, 33, 40}, seed++, 1);
    }
    run_overlap_add(5, 1, 0, {1, 2, 8}, seed++, 0);
}

// ---- refusals -----------------------------------------------------------------
void run_rejections()
{
    Buf ring(64, 0), m(64, 0), z(64, 0), f(8, 0), c(8, 0), y(64, 0);
    // W 8, O 2: H 6; a ring of 20 holding [0, 20): windows 0, 1, 2 are regular (2 ends at 20)
#define GATHER(ring_, cap, lo, fed, W, O, first, count, slots, closing, T, rows, win, mix, mbs, nz, nrs, nbs) \
    ou_stream_gather(ring_, cap, lo, fed, W, O, first, count, slots, closing, T, rows, win, 1, 0, mix, mbs, nz, nrs, nbs, nullptr)
    OK(GATHER(ring.p, 20, 0, 20, 8, 2, 0, 3, 3, 0, 0, 2, 9, m.p, 8, z.p, 27, 9));
    OK(GATHER(ring.p, 20, 0, 20, 8, 2, 0, 3, 3, 1, 20, 2, 9, m.p, 8, z.p, 27, 9));    // closing, nothing shifted
    OK(GATHER(ring.p, 20, 0, 19, 8, 2, 1, 2, 3, 1, 19, 2, 9, m.p, 8, z.p, 27, 9));    // closing, window 2 at 11
    OK(GATHER(ring.p, 20, 0, 20, 8, 2, 0, 2, 2, 0, 0, 0, 0, m.p, 8, nullptr, 0, 0));  // no noise rows: no NZ
    REFUSED(GATHER(nullptr, 20, 0, 20, 8, 2, 0, 3, 3, 0, 0, 2, 9, m.p, 8, z.p, 27, 9));
    REFUSED(GATHER(ring.p, 20, 0, 20, 8, 2, 0, 3, 3, 0, 0, 2, 9, nullptr, 8, z.p, 27, 9));
    REFUSED(GATHER(ring.p, 20, 0, 20, 8, 2, 0, 3, 3, 0, 0, 2, 9, m.p, 8, nullptr, 27, 9));
    REFUSED(GATHER(ring.p, 20, 0, 20, 0, 0, 0, 3, 3, 0, 0, 2, 9, m.p, 8, z.p, 27, 9));     // W
    REFUSED(GATHER(ring.p, 20, 0, 20, 8, 5, 0, 3, 3, 0, 0, 2, 9, m.p, 8, z.p, 27, 9));     // O > W / 2
    REFUSED(GATHER(ring.p, 20, 0, 20, 8, -1, 0, 3, 3, 0, 0, 2, 9, m.p, 8, z.p, 27, 9));
    REFUSED(GATHER(ring.p, 20, 0, 20, 8, 2, -1, 3, 3, 0, 0, 2, 9, m.p, 8, z.p, 27, 9));    // first
    REFUSED(GATHER(ring.p, 20, 0, 20, 8, 2, 0, 0, 3, 0, 0, 2, 9, m.p, 8, z.p, 27, 9));     // count
    REFUSED(GATHER(ring.p, 20, 0, 20, 8, 2, 0, 3, 2, 0, 0, 2, 9, m.p, 8, z.p, 27, 9));     // slots < count
    REFUSED(GATHER(ring.p, 20, 0, 20, 8, 2, 0, 3, 3, 0, 0, -1, 9, m.p, 8, z.p, 27, 9));    // rows
    REFUSED(GATHER(ring.p, 20, 0, 20, 8, 2, 0, 3, 3, 0, 0, 2, 0, m.p, 8, z.p, 27, 9));     // noise_win
    REFUSED(GATHER(ring.p, 7, 0, 7, 8, 2, 0, 1, 1, 0, 0, 2, 9, m.p, 8, z.p, 27, 9));       // cap < W
    REFUSED(GATHER(ring.p, 20, -1, 19, 8, 2, 0, 3, 3, 0, 0, 2, 9, m.p, 8, z.p, 27, 9));    // lo
    REFUSED(GATHER(ring.p, 20, 0, 21, 8, 2, 0, 3, 3, 0, 0, 2, 9, m.p, 8, z.p, 27, 9));     // fed - lo > cap
    REFUSED(GATHER(ring.p, 20, 21, 20, 8, 2, 0, 3, 3, 0, 0, 2, 9, m.p, 8, z.p, 27, 9));    // fed < lo
    REFUSED(GATHER(ring.p, 20, 0, 19, 8, 2, 0, 3, 3, 0, 0, 2, 9, m.p, 8, z.p, 27, 9));     // window 2 ends past fed
    REFUSED(GATHER(ring.p, 20, 1, 20, 8, 2, 0, 3, 3, 0, 0, 2, 9, m.p, 8, z.p, 27, 9));     // window 0 starts below lo
    REFUSED(GATHER(ring.p, 20, 0, 20, 8, 2, 0, 3, 3, 1, 19, 2, 9, m.p, 8, z.p, 27, 9));    // closing: T != fed
    REFUSED(GATHER(ring.p, 20, 0, 20, 8, 2, 0, 2, 3, 1, 20, 2, 9, m.p, 8, z.p, 27, 9));    // closing: T has 3 windows
    REFUSED(GATHER(ring.p, 20, 0, 7, 8, 2, 0, 1, 1, 1, 7, 2, 9, m.p, 8, z.p, 27, 9));      // closing: T < W
    REFUSED(GATHER(ring.p, 20, 0, 20, 8, 2, 0, 3, 3, 0, 0, 2, 9, m.p, 7, z.p, 27, 9));     // MIX rows overlap
    REFUSED(GATHER(ring.p, 20, 0, 20, 8, 2, 0, 3, 3, 0, 0, 2, 9, m.p, 8, z.p, 27, 8));     // NZ items overlap
    REFUSED(GATHER(ring.p, 20, 0, 20, 8, 2, 0, 3, 3, 0, 0, 2, 9, m.p, 8, z.p, 26, 9));     // NZ rows overlap
    {   // noise past sample 2^40: with O = 0, H = 8 and the last window of 2^40 samples starts at 2^40 - 8
        const long long fed = 1LL << 40;
        REFUSED(GATHER(ring.p, 20, fed - 20, fed, 8, 0, (fed - 8) / 8, 1, 1, 0, 0, 2, 9, m.p, 8, z.p, 27, 9));
        OK(GATHER(ring.p, 20, fed - 20, fed, 8, 0, (fed - 8) / 8, 1, 1, 0, 0, 2, 8, m.p, 8, z.p, 27, 9));
    }

#define OADD(w, wbs, W, O, first, count, closing, T, fade, carry, out) \
    ou_stream_overlap_add(w, wbs, W, O, first, count, closing, T, fade, carry, out, nullptr, nullptr)
    OK(OADD(m.p, 8, 8, 2, 0, 3, 0, 0, f.p, c.p, y.p));
    OK(OADD(m.p, 8, 8, 2, 3, 0, 1, 20, f.p, c.p, y.p));                       // closing from the carry alone
    OK(OADD(m.p, 8, 8, 0, 0, 3, 0, 0, nullptr, nullptr, y.p));                // O = 0 needs neither table nor carry
    OK(OADD(nullptr, 8, 8, 0, 3, 0, 1, 24, nullptr, nullptr, nullptr));       // O = 0, nothing left: nothing to emit
    REFUSED(OADD(nullptr, 8, 8, 2, 0, 3, 0, 0, f.p, c.p, y.p));
    REFUSED(OADD(m.p, 8, 8, 2, 0, 3, 0, 0, f.p, c.p, nullptr));
    REFUSED(OADD(m.p, 8, 8, 2, 0, 3, 0, 0, nullptr, c.p, y.p));               // O > 0 needs the table
    REFUSED(OADD(m.p, 8, 8, 2, 0, 3, 0, 0, f.p, nullptr, y.p));               // and the carry
    REFUSED(OADD(m.p, 8, 0, 0, 0, 3, 0, 0, f.p, c.p, y.p));                   // W
    REFUSED(OADD(m.p, 8, 8, 5, 0, 3, 0, 0, f.p, c.p, y.p));                   // O > W / 2
    REFUSED(OADD(m.p, 8, 8, -1, 0, 3, 0, 0, f.p, c.p, y.p));
    REFUSED(OADD(m.p, 8, 8, 2, -1, 3, 0, 0, f.p, c.p, y.p));                  // first
    REFUSED(OADD(m.p, 8, 8, 2, 0, 0, 0, 0, f.p, c.p, y.p));                   // count < 1 and not closing
    REFUSED(OADD(m.p, 8, 8, 2, 0, -1, 1, 8, f.p, c.p, y.p));
    REFUSED(OADD(m.p, 7, 8, 2, 0, 3, 0, 0, f.p, c.p, y.p));                   // windows overlap in w
    REFUSED(OADD(m.p, 8, 8, 2, 0, 1, 1, 7, f.p, c.p, y.p));                   // closing: T < W
    REFUSED(OADD(m.p, 8, 8, 2, 0, 2, 1, 20, f.p, c.p, y.p));                  // closing: T has 3 windows
    REFUSED(OADD(m.p, 8, 8, 2, 3, 0, 1, 19, f.p, c.p, y.p));                  // closing without windows: window 2 shifted
    REFUSED(OADD(m.p, 8, 8, 2, 1, 3, 1, 20, f.p, c.p, y.p));
}

}  // namespace

int main()
{
    run_gathers();
    run_overlap_adds();
    run_rejections();
    std::printf("ok: %d launches checked, %d calls refused\n", g_launches, g_refusals);
    return 0;
}
