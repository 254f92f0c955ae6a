// The pooled windows' kernels (ou_pool.hip) on the CPU: the HIP source compiled
// for the host against tests/emu/hip/hip_runtime.h, under AddressSanitizer,
// every workgroup run (OUHIP_EMU_BLOCKS=0).  Every buffer is an exact-size heap
// block, so an access outside an array aborts with its location.  The kernels
// have no barriers and no LDS, and within one call no thread reads what
// another stores, so the emulated values are real.  They are checked against a
// host restatement of the definition (include/ouhip.h): the gather bit for
// bit, poison between the rows intact; the overlap-add, from results that
// start as NaN, bit for bit against the per-sample rule
//   own = min(t / H, n_c - 1);  y[t] = (0 + (1 - f) v_{own-1}) + f v_own
// inside the owner's fade-in and 0 + 1 v_own elsewhere, for every grouping.
// The shapes are those of tests/test_gpu_long_pool.py, then small windows that
// are no multiple of four and a call of more than 32 slots.  Last, every entry
// point must refuse what the header says it refuses.
#include "../../open_universe_amd/csrc/ou_pool.hip"

#include <cmath>
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

// ---- the host restatement -------------------------------------------------
struct Clip {
    long long T, n;
    std::vector<long long> st;
    Clip(long long T_, int W, int O) : T(T_)
    {
        const long long H = W - O;
        n = 1 + (T - W + H - 1) / H;
        for (long long i = 0; i < n; ++i) st.push_back(std::min(i * H, T - W));
    }
};

struct Pool {
    int W, O;
    std::vector<Clip> clips;
    std::vector<std::pair<int, long long>> slots;   // (c, i)
    Pool(std::vector<long long> Ts, int W_, int O_) : W(W_), O(O_)
    {
        for (long long T : Ts) clips.emplace_back(T, W, O);
        for (size_t c = 0; c < clips.size(); ++c)
            for (long long i = 0; i < clips[c].n; ++i) slots.emplace_back((int)c, i);
    }
    long long N() const { return (long long)slots.size(); }
    std::pair<int, long long> slot(long long s) const { return slots[(size_t)std::min(s, N() - 1)]; }
    long long start(long long s) const { return clips[slot(s).first].st[(size_t)slot(s).second]; }
};

void run_gather(const Pool& p, long long first, int count, int rows, long long win, long long gap, int mis_x,
                int mis_y)
{
    const int C = (int)p.clips.size(), W = p.W;
    std::vector<Buf*> xs, ns;
    std::vector<ou_pool_clip> cl((size_t)C);
    for (int c = 0; c < C; ++c) {
        const Clip& k = p.clips[c];
        const long long nrs = k.st.back() + win + (c % 2 ? 3 : 0);   // the rows' bases differ mod 4
        xs.push_back(new Buf((size_t)k.T, (mis_x + c) % 4));
        ns.push_back(new Buf(rows ? (size_t)((rows - 1) * nrs + k.st.back() + win) : 1, (mis_x + 2 * c) % 4));
        for (size_t i = 0; i < xs[c]->n; ++i) xs[c]->p[i] = (float)((i + 7919 * c) % 65521) * 0.25f - 100.f;
        for (size_t i = 0; i < ns[c]->n; ++i) ns[c]->p[i] = (float)((i + 104729 * c) % 65519) * -0.5f + 3.f;
        cl[c] = ou_pool_clip{xs[c]->p, rows ? ns[c]->p : nullptr, nullptr, k.T, nrs};
    }
    const long long mbs = W + gap, nbs = win + gap, nrs_out = count * nbs + 5;
    Buf mix((size_t)((count - 1) * mbs + W), mis_y, kPoison);
    Buf nz(rows ? (size_t)((rows - 1) * nrs_out + (count - 1) * nbs + win) : 1, mis_y, kPoison);
    OK(ou_pool_gather(cl.data(), C, W, p.O, first, count, rows, win, mix.p, mbs, rows ? nz.p : nullptr, nrs_out, nbs,
                      nullptr));
    std::vector<char> wm(mix.n, 0), wn(nz.n, 0);
    for (int b = 0; b < count; ++b) {
        const int c = p.slot(first + b).first;
        const long long s = p.start(first + b);
        for (long long j = 0; j < W; ++j) {
            const size_t i = (size_t)(b * mbs + j);
            CHECK(mix.p[i] == xs[c]->p[s + j], "mix: slot %lld sample %lld: %g != %g", first + b, j, mix.p[i],
                  xs[c]->p[s + j]);
            wm[i] = 1;
        }
        for (int r = 0; r < rows; ++r)
            for (long long j = 0; j < win; ++j) {
                const size_t i = (size_t)(r * nrs_out + b * nbs + j);
                const float want = ns[c]->p[r * cl[c].noise_rstride + s + j];
                CHECK(nz.p[i] == want, "nz: row %d slot %lld sample %lld: %g != %g", r, first + b, j, nz.p[i], want);
                wn[i] = 1;
            }
    }
    for (size_t i = 0; i < mix.n; ++i) CHECK(wm[i] || mix.p[i] == kPoison, "mix[%zu] between the rows was written", i);
    if (rows)
        for (size_t i = 0; i < nz.n; ++i) CHECK(wn[i] || nz.p[i] == kPoison, "nz[%zu] between the rows was written", i);
    for (Buf* b : xs) delete b;
    for (Buf* b : ns) delete b;
}

void run_gathers()
{
    const Pool p({9000, 4001, 10400}, 4000, 800);   // 3 + 2 + 3 slots
    CHECK(p.N() == 8, "N %lld", p.N());
    // the ragged last lane where source and destination both end with the row, at 16-byte aligned bases:
    // an unguarded 16-byte access leaves the blocks
    run_gather(p, 7, 1, 1, 4163, 0, 0, 0);
    for (long long win : {4160LL, 4163LL})
        for (int mis = 0; mis < 4; ++mis) {
            run_gather(p, 0, 3, 3, win, 0, mis, 0);       // one clip's windows
            run_gather(p, 3, 3, 3, win, 36, 0, mis);      // a group that straddles two clips
            run_gather(p, 6, 3, 3, win, 1, mis, mis);     // a group that runs past N: the clamp
            run_gather(p, 0, 8, 3, win, 0, mis, 1);
        }
    run_gather(p, 2, 4, 0, 4160, 8, 1, 0);                // no noise rows: MIX alone
    run_gather(p, 7, 1, 1, 4000, 0, 0, 0);
    const Pool q({700, 38, 700, 101}, 37, 5);             // W % 4 != 0; 22 + 2 + 22 + 3 slots
    CHECK(q.N() == 49, "N %lld", q.N());
    run_gather(q, 0, 49, 2, 41, 0, 1, 2);                 // more than 32 slots: two launches
    run_gather(q, 20, 40, 3, 37, 3, 0, 0);                // and past N
    run_gather(q, 48, 33, 1, 64, 0, 3, 1);                // every slot the clamped one
}

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

// all groupings of `counts` over the clips Ts; every y starts as NaN, clip 1's is misaligned by 1
void run_overlap_add(std::vector<long long> Ts, int W, int O, std::vector<int> counts, unsigned seed)
{
    const Pool p(Ts, W, O);
    const int C = (int)p.clips.size();
    const long long N = p.N(), H = W - O, bs = W + 8;
    Buf w((size_t)((N - 1) * bs + W), 1);
    std::mt19937 gen(seed);
    std::uniform_real_distribution<float> dist(-1.f, 1.f);
    for (size_t i = 0; i < w.n; ++i) w.p[i] = dist(gen);
    const std::vector<float> fade = fade_table(O);
    Buf tab((size_t)2 * O + (O ? 0 : 1), 0);
    for (int i = 0; i < 2 * O; ++i) tab.p[i] = fade[i];
    const float* ft = O ? tab.p : nullptr;

    // the per-sample rule
    std::vector<std::vector<float>> want((size_t)C);
    long long s0 = 0;   // the clip's first slot
    for (int c = 0; c < C; ++c) {
        const Clip& k = p.clips[c];
        for (long long t = 0; t < k.T; ++t) {
            const long long own = std::min(t / H, k.n - 1), u = t - own * H;
            const float v = w.p[(s0 + own) * bs + (t - k.st[own])];
            float y;
            if (own > 0 && u < O) {
                const float vp = w.p[(s0 + own - 1) * bs + (t - k.st[own - 1])];
                y = (0.f + fade[O + u] * vp) + fade[u] * v;
            } else {
                y = 0.f + 1.f * v;
            }
            want[c].push_back(y);
        }
        s0 += k.n;
    }

    for (int count : counts) {
        std::vector<Buf*> ys;
        std::vector<ou_pool_clip> cl((size_t)C);
        for (int c = 0; c < C; ++c) {
            ys.push_back(new Buf((size_t)p.clips[c].T, c == 1 ? 1 : 0, std::numeric_limits<float>::quiet_NaN()));
            cl[c] = ou_pool_clip{nullptr, nullptr, ys[c]->p, p.clips[c].T, 0};
        }
        const int cnt = count > 0 ? count : (int)N;
        for (long long first = 0; first < N; first += cnt)   // the last call's count runs past N: ignored
            OK(ou_pool_overlap_add(cl.data(), C, W, O, first, cnt, w.p + first * bs, bs, ft, nullptr));
        for (int c = 0; c < C; ++c) {
            for (long long t = 0; t < p.clips[c].T; ++t)
                CHECK(std::memcmp(&ys[c]->p[t], &want[c][t], 4) == 0, "W %d O %d count %d clip %d sample %lld: %.9g != %.9g",
                      W, O, cnt, c, t, ys[c]->p[t], want[c][t]);
            delete ys[c];
        }
    }
}

void run_overlap_adds()
{
    unsigned seed = 1;
    for (int O : {800, 0, 2000}) run_overlap_add({9000, 4001, 10400}, 4000, O, {1, 2, 3, 5, 0}, seed++);
    run_overlap_add({10397, 4001}, 4000, 800, {1, 2, 0}, seed++);   // a last window shifted by less than the overlap
    for (int O : {18, 5, 0}) run_overlap_add({700, 38, 700, 101}, 37, O, {1, 2, 3, 5, 33, 40, 0}, seed++);
    run_overlap_add({5, 2}, 1, 0, {1, 2, 0}, seed++);
}

void run_rejections()
{
    Buf a(64, 0), b(64, 0), n(64, 0), f(8, 0), m(64, 0), z(64, 0);
    // two clips of 20 and 9 samples, W 8, O 2: H 6, 3 + 2 slots; noise rows of 12 + 9 = 21 and 1 + 9 = 10 values
    ou_pool_clip cl[2] = {{a.p, n.p, b.p, 20, 21}, {a.p + 32, n.p, b.p + 32, 9, 10}};
    const int64_t Ts[2] = {20, 9};
    int64_t N = 0;
    OK(ou_pool_slots(Ts, 2, 8, 2, &N));
    CHECK(N == 5, "N %lld", (long long)N);
    REFUSED(ou_pool_slots(nullptr, 2, 8, 2, &N));
    REFUSED(ou_pool_slots(Ts, 0, 8, 2, &N));
    REFUSED(ou_pool_slots(Ts, 2, 9, 2, &N));       // T = window: such a clip is one plain enhance
    REFUSED(ou_pool_slots(Ts, 2, 10, 2, &N));      // T < window
    REFUSED(ou_pool_slots(Ts, 2, 0, 0, &N));
    REFUSED(ou_pool_slots(Ts, 2, 8, 5, &N));       // O > W / 2
    REFUSED(ou_pool_slots(Ts, 2, 8, -1, &N));

#define GATHER(cl_, nc, W, O, first, count, rows, win, mix, mbs, nz, nrs, nbs) \
    ou_pool_gather(cl_, nc, W, O, first, count, rows, win, mix, mbs, nz, nrs, nbs, nullptr)
    OK(GATHER(cl, 2, 8, 2, 3, 3, 2, 9, m.p, 8, z.p, 27, 9));
    OK(GATHER(cl, 2, 8, 2, 0, 2, 0, 0, m.p, 8, nullptr, 0, 0));   // no noise rows: no NZ, no noise pointers
    REFUSED(GATHER(nullptr, 2, 8, 2, 0, 3, 2, 9, m.p, 8, z.p, 27, 9));
    REFUSED(GATHER(cl, 0, 8, 2, 0, 3, 2, 9, m.p, 8, z.p, 27, 9));
    REFUSED(GATHER(cl, 2, 8, 2, 0, 3, 2, 9, nullptr, 8, z.p, 27, 9));
    REFUSED(GATHER(cl, 2, 8, 2, 0, 3, 2, 9, m.p, 8, nullptr, 27, 9));
    REFUSED(GATHER(cl, 2, 9, 2, 0, 3, 2, 9, m.p, 9, z.p, 27, 9));      // T <= window
    REFUSED(GATHER(cl, 2, 8, 5, 0, 3, 2, 9, m.p, 8, z.p, 27, 9));      // O > W / 2
    REFUSED(GATHER(cl, 2, 8, -1, 0, 3, 2, 9, m.p, 8, z.p, 27, 9));
    REFUSED(GATHER(cl, 2, 8, 2, -1, 3, 2, 9, m.p, 8, z.p, 27, 9));     // first
    REFUSED(GATHER(cl, 2, 8, 2, 5, 3, 2, 9, m.p, 8, z.p, 27, 9));
    REFUSED(GATHER(cl, 2, 8, 2, 0, 0, 2, 9, m.p, 8, z.p, 27, 9));      // count
    REFUSED(GATHER(cl, 2, 8, 2, 0, 3, -1, 9, m.p, 8, z.p, 27, 9));     // rows
    REFUSED(GATHER(cl, 2, 8, 2, 0, 3, 2, 0, m.p, 8, z.p, 27, 9));      // noise_win
    REFUSED(GATHER(cl, 2, 8, 2, 0, 3, 2, 9, m.p, 7, z.p, 27, 9));      // MIX rows overlap
    REFUSED(GATHER(cl, 2, 8, 2, 0, 3, 2, 9, m.p, 8, z.p, 27, 8));      // NZ items overlap
    REFUSED(GATHER(cl, 2, 8, 2, 0, 3, 2, 9, m.p, 8, z.p, 26, 9));      // NZ rows overlap
    REFUSED(GATHER(cl, 2, 8, 2, 0, 3, 2, 10, m.p, 8, z.p, 30, 10));    // noise_rstride < start_last + noise_win
    {
        ou_pool_clip bad[2] = {cl[0], cl[1]};
        bad[1].x = nullptr;
        REFUSED(GATHER(bad, 2, 8, 2, 0, 3, 2, 9, m.p, 8, z.p, 27, 9));
        bad[1] = cl[1], bad[0].noise = nullptr;
        REFUSED(GATHER(bad, 2, 8, 2, 0, 3, 2, 9, m.p, 8, z.p, 27, 9));
        bad[0] = cl[0], bad[0].noise_rstride = 20;
        REFUSED(GATHER(bad, 2, 8, 2, 0, 3, 2, 9, m.p, 8, z.p, 27, 9));
    }

#define OADD(cl_, nc, W, O, first, count, w, wbs, fade) ou_pool_overlap_add(cl_, nc, W, O, first, count, w, wbs, fade, nullptr)
    OK(OADD(cl, 2, 8, 2, 0, 5, m.p, 8, f.p));
    OK(OADD(cl, 2, 8, 0, 0, 5, m.p, 8, nullptr));                      // O = 0 needs no table
    REFUSED(OADD(nullptr, 2, 8, 2, 0, 5, m.p, 8, f.p));
    REFUSED(OADD(cl, -1, 8, 2, 0, 5, m.p, 8, f.p));
    REFUSED(OADD(cl, 2, 8, 2, 0, 5, nullptr, 8, f.p));
    REFUSED(OADD(cl, 2, 8, 2, 0, 5, m.p, 8, nullptr));                 // O > 0 needs the table
    REFUSED(OADD(cl, 2, 9, 2, 0, 5, m.p, 9, f.p));                     // T <= window
    REFUSED(OADD(cl, 2, 8, 5, 0, 5, m.p, 8, f.p));                     // O > W / 2
    REFUSED(OADD(cl, 2, 8, -1, 0, 5, m.p, 8, f.p));
    REFUSED(OADD(cl, 2, 8, 2, -1, 5, m.p, 8, f.p));                    // first
    REFUSED(OADD(cl, 2, 8, 2, 5, 1, m.p, 8, f.p));
    REFUSED(OADD(cl, 2, 8, 2, 0, 0, m.p, 8, f.p));                     // count
    REFUSED(OADD(cl, 2, 8, 2, 0, 5, m.p, 7, f.p));                     // windows overlap in w
    {
        ou_pool_clip bad[2] = {cl[0], cl[1]};
        bad[1].y = nullptr;
        REFUSED(OADD(bad, 2, 8, 2, 0, 5, m.p, 8, f.p));
        bad[1].y = b.p + 19;                                           // the results share one sample
        REFUSED(OADD(bad, 2, 8, 2, 0, 5, m.p, 8, f.p));
        bad[1].y = b.p + 20;
        OK(OADD(bad, 2, 8, 2, 0, 5, m.p, 8, f.p));
        bad[0].y = b.p + 5, bad[1].y = b.p;                            // in the other order
        REFUSED(OADD(bad, 2, 8, 2, 0, 5, m.p, 8, f.p));
    }
}

// lengths past 2^31 samples: the arithmetic alone
void run_past_2_31()
{
    const int64_t Ts[2] = {(1LL << 31) + 12345, 9000}, W = 4000, O = 800, H = W - O;
    int64_t N = 0;
    OK(ou_pool_slots(Ts, 2, (int)W, (int)O, &N));
    CHECK(N == 1 + (Ts[0] - W + H - 1) / H + 3 && N > 671000, "N %lld", (long long)N);
    PoolGeom g;
    ou_pool_clip cl[2] = {{nullptr, nullptr, nullptr, Ts[0], 0}, {nullptr, nullptr, nullptr, Ts[1], 0}};
    CHECK(pool_geom("t", nullptr, cl, 2, (int)W, (int)O, &g) == 0 && g.N == N, "geometry");
    PoolWalk at(cl, g, N - 4);
    CHECK(at.c == 0 && at.i == N - 4 && at.start() == Ts[0] - W && at.start() > (1LL << 31), "start %lld", at.start());
    at.next();
    CHECK(at.c == 1 && at.i == 0 && at.start() == 0, "the next clip");
    at.next(), at.next();
    CHECK(at.c == 1 && at.i == 2 && at.start() == 5000 && at.left == 0, "the last slot");
    at.next();
    CHECK(at.c == 1 && at.i == 2, "the clamp");
}

}  // namespace

int main()
{
    run_gathers();
    run_overlap_adds();
    run_rejections();
    run_past_2_31();
    std::printf("ok: %d launches checked, %d calls refused\n", g_launches, g_refusals);
    return 0;
}
