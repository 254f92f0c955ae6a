// The windowed enhance's kernels (ou_long.hip) on the CPU: the HIP source
// compiled for the host against tests/emu/hip/hip_runtime.h, under
// AddressSanitizer, every workgroup run (OUHIP_EMU_BLOCKS=0).  Every buffer is
// an exact-size heap block, so an access outside an array aborts with its
// location.  The kernels have no barriers and no LDS: each thread computes
// its own samples, so the values are real and are checked against a host
// restatement of the definition (include/ouhip.h) -- the gather bit for bit,
// the overlap-add against a double evaluation, and split into calls against
// one call bit for bit.  The shapes are those of tests/test_gpu_long.py, at
// aligned and misaligned bases.  Then both entry points must refuse what the
// header says they refuse, and one geometry past 2^31 samples is checked
// through the arguments alone (nothing is allocated or launched).
#include "../../open_universe_amd/csrc/ou_long.hip"

#include <random>
#include <string>

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
        if ((call) == 0) {                                                                    \
            std::fprintf(stderr, "%s:%d: %s was accepted\n", __FILE__, __LINE__, #call);      \
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
        // the block ends with the last float; its start is 16-byte aligned (malloc) plus the misalignment
        raw = (char*)std::malloc((n + mis) * sizeof(float));
        p = (float*)raw + mis;
        for (size_t i = 0; i < n; ++i) p[i] = fill;
    }
    ~Buf() { std::free(raw); }
    Buf(const Buf&) = delete;
};

// ---- the host restatement -------------------------------------------------
struct Ref {
    long long T, n, H;
    int W, O;
    Ref(long long T_, int W_, int O_) : T(T_), W(W_), O(O_)
    {
        H = W - O;
        n = T <= W ? 1 : 1 + (T - W + H - 1) / H;
    }
    long long start(long long i) const
    {
        if (i > n - 1) i = n - 1;
        return std::min(i * H, T - W);
    }
    // weight of window i at sample t, in double
    double weight(long long i, long long t) const
    {
        const long long s = start(i);
        if (t < s || t >= s + W) return 0.0;
        const double pi = 3.14159265358979323846;
        if (i >= 1) {
            const long long lo = start(i - 1) + W - O;   // fade-in of window i
            if (t < lo) return 0.0;
            if (t < lo + O) {
                const double sn = std::sin(pi * (2.0 * (t - lo) + 1.0) / (4.0 * O));
                return sn * sn;
            }
        }
        if (i + 1 < n) {
            const long long lo = s + W - O;              // fade-in of window i + 1
            if (t >= lo + O) return 0.0;
            if (t >= lo) {
                const double sn = std::sin(pi * (2.0 * (t - lo) + 1.0) / (4.0 * O));
                return 1.0 - sn * sn;
            }
        }
        return 1.0;
    }
};

const float kPoison = 1e6f;

void run_gather(long long T, int W, int O, int rows, long long win, long long first, int count, long long y_gap,
                int mis_x, int mis_y)
{
    const Ref r(T, W, O);
    const long long row = (T - W) + win, xrs = rows > 1 ? row + 5 : 0;
    Buf x((size_t)((rows - 1) * xrs + row), mis_x);
    for (size_t i = 0; i < x.n; ++i) x.p[i] = (float)(i % 65521) * 0.25f - 100.f;
    const long long ybs = win + y_gap, yrs = rows > 1 ? count * ybs + 3 : 0;
    Buf y((size_t)((rows - 1) * yrs + (count - 1) * ybs + win), mis_y, kPoison);
    OK(ou_window_gather(x.p, xrs, rows, T, W, O, first, count, win, y.p, yrs, ybs, nullptr));
    std::vector<char> written(y.n, 0);
    for (int rr = 0; rr < rows; ++rr)
        for (int b = 0; b < count; ++b)
            for (long long j = 0; j < win; ++j) {
                const size_t yi = (size_t)(rr * yrs + b * ybs + j);
                const float want = x.p[rr * xrs + r.start(first + b) + j];
                CHECK(y.p[yi] == want, "T %lld row %d item %d sample %lld: %g != %g", T, rr, b, j, y.p[yi], want);
                written[yi] = 1;
            }
    for (size_t i = 0; i < y.n; ++i) CHECK(written[i] || y.p[i] == kPoison, "y[%zu] outside every item was written", i);
}

void run_gathers()
{
    const int W = 4000, O = 800;
    for (long long T : {4001LL, 9000LL, 10400LL}) {
        const Ref r(T, W, O);
        for (int rows : {1, 7})
            for (int mis = 0; mis < 4; mis += (rows == 1 ? 1 : 3)) {
                // first + b runs past n (the clamp): 4 items from window 0, 2 from the last
                run_gather(T, W, O, rows, W, 0, 4, 0, mis, 0);
                run_gather(T, W, O, rows, W, r.n - 1, 2, 160, 0, mis);    // a destination stride larger than win
                run_gather(T, W, O, rows, 4160, 0, 2, 0, mis, mis);       // the noise: win = the padded length
            }
    }
    run_gather(9000, 4000, 0, 1, 4000, 1, 2, 0, 1, 2);
    run_gather(9000, 4000, 2000, 2, 4003, 1, 3, 1, 2, 1);                 // win % 4 != 0: the ragged last lanes
    run_gather(4000, 4000, 800, 1, 4000, 0, 1, 0, 0, 0);                  // one window: T = W
    run_gather(23, 7, 3, 3, 9, 2, 4, 0, 0, 0);
    run_gather(5, 1, 0, 1, 1, 3, 2, 0, 0, 0);
}

void run_overlap_add(long long T, int W, int O, int mis_y, unsigned seed)
{
    const Ref r(T, W, O);
    const int n = (int)r.n;
    const long long bs = W + 8;
    Buf w((size_t)((n - 1) * bs + W), 1);
    std::mt19937 gen(seed);
    std::uniform_real_distribution<float> dist(-1.f, 1.f);
    for (size_t i = 0; i < w.n; ++i) w.p[i] = dist(gen);
    std::vector<float> fade(2 * (size_t)O + 1);
    CHECK(ou_long_fade(O, fade.data()) == 0, "%s", ouhip_detail::err_buf());
    Buf tab((size_t)2 * O, 0);
    for (int i = 0; i < 2 * O; ++i) tab.p[i] = fade[i];
    const float* ft = O ? tab.p : nullptr;

    // one call for all windows (count past n: ignored)
    Buf y1((size_t)T, mis_y, kPoison);
    OK(ou_overlap_add(w.p, bs, T, W, O, 0, n + 2, ft, y1.p, nullptr));
    double emax = 0, ymax = 0;
    for (long long t = 0; t < T; ++t) {
        double ref = 0;
        int nz = 0;
        for (int i = 0; i < n; ++i) {
            const double wt = r.weight(i, t);
            if (wt != 0) ref += wt * (double)w.p[i * bs + (t - r.start(i))], ++nz;
        }
        CHECK(nz >= 1 && nz <= 2, "%d windows at sample %lld", nz, t);
        emax = std::max(emax, std::fabs((double)y1.p[t] - ref));
        ymax = std::max(ymax, std::fabs(ref));
    }
    // two products and one sum, each rounded once, of weights rounded once: 4 half-ulps of the largest value
    CHECK(emax <= 4 * 0x1p-24 * std::max(ymax, 1.0), "T %lld O %d: error %g", T, O, emax);

    // window by window, and in groups of two: the same bits
    for (int step : {1, 2}) {
        Buf y2((size_t)T, mis_y, kPoison);
        for (int first = 0; first < n; first += step)
            OK(ou_overlap_add(w.p + first * bs, bs, T, W, O, first, step, ft, y2.p, nullptr));
        CHECK(std::memcmp(y1.p, y2.p, (size_t)T * 4) == 0, "T %lld O %d: split by %d differs", T, O, step);
    }

    // a constant 1.0 comes back within one ulp of 1
    for (size_t i = 0; i < w.n; ++i) w.p[i] = 1.f;
    OK(ou_overlap_add(w.p, bs, T, W, O, 0, n, ft, y1.p, nullptr));
    for (long long t = 0; t < T; ++t)
        CHECK(std::fabs((double)y1.p[t] - 1.0) <= 0x1p-23, "T %lld O %d: ones give %.9g at %lld", T, O, y1.p[t], t);
}

void run_overlap_adds()
{
    unsigned seed = 1;
    for (long long T : {4001LL, 9000LL, 10400LL})
        for (int O : {800, 0, 2000})
            for (int mis : {0, 1}) run_overlap_add(T, 4000, O, mis, seed++);
    run_overlap_add(4000, 4000, 800, 0, seed++);
    run_overlap_add(10397, 4000, 800, 3, seed++);   // the last window shifted by less than the overlap
    run_overlap_add(23, 7, 3, 2, seed++);
    run_overlap_add(5, 1, 0, 0, seed++);
}

void run_rejections()
{
    Buf a(64, 0), b(64, 0), f(8, 0);
    float *x = a.p, *y = b.p;
    // T 20, W 8, O 2: H 6, n 3
    OK(ou_window_gather(x, 0, 1, 20, 8, 2, 2, 2, 8, y, 0, 8, nullptr));
    REFUSED(ou_window_gather(nullptr, 0, 1, 20, 8, 2, 0, 2, 8, y, 0, 8, nullptr));
    REFUSED(ou_window_gather(x, 0, 1, 20, 8, 2, 0, 2, 8, nullptr, 0, 8, nullptr));
    REFUSED(ou_window_gather(x, 0, 0, 20, 8, 2, 0, 2, 8, y, 0, 8, nullptr));     // rows
    REFUSED(ou_window_gather(x, 0, -1, 20, 8, 2, 0, 2, 8, y, 0, 8, nullptr));
    REFUSED(ou_window_gather(x, 0, 1, 20, 8, 2, 0, 0, 8, y, 0, 8, nullptr));     // count
    REFUSED(ou_window_gather(x, 0, 1, 20, 8, 2, 0, 2, 0, y, 0, 8, nullptr));     // win
    REFUSED(ou_window_gather(x, 0, 1, 20, 0, 0, 0, 2, 8, y, 0, 8, nullptr));     // window
    REFUSED(ou_window_gather(x, 0, 1, 20, -8, 0, 0, 2, 8, y, 0, 8, nullptr));
    REFUSED(ou_window_gather(x, 0, 1, 20, 8, 5, 0, 2, 8, y, 0, 8, nullptr));     // O > W / 2
    REFUSED(ou_window_gather(x, 0, 1, 20, 8, -1, 0, 2, 8, y, 0, 8, nullptr));
    REFUSED(ou_window_gather(x, 0, 1, 0, 8, 2, 0, 2, 8, y, 0, 8, nullptr));      // T < 1
    REFUSED(ou_window_gather(x, 0, 1, -20, 8, 2, 0, 2, 8, y, 0, 8, nullptr));
    REFUSED(ou_window_gather(x, 0, 1, 7, 8, 2, 0, 2, 8, y, 0, 8, nullptr));      // T < W
    REFUSED(ou_window_gather(x, 0, 1, 20, 8, 2, -1, 2, 8, y, 0, 8, nullptr));    // first < 0
    REFUSED(ou_window_gather(x, 0, 1, 20, 8, 2, 3, 2, 8, y, 0, 8, nullptr));     // a group past the end
    REFUSED(ou_window_gather(x, 0, 1, 20, 8, 2, 0, 2, 8, y, 0, 7, nullptr));     // items overlap
    REFUSED(ou_window_gather(x, 19, 2, 20, 8, 2, 0, 2, 8, y, 16, 8, nullptr));   // source rows overlap
    REFUSED(ou_window_gather(x, 20, 2, 20, 8, 2, 0, 2, 8, y, 15, 8, nullptr));   // destination rows overlap

    OK(ou_overlap_add(x, 8, 20, 8, 2, 0, 3, f.p, y, nullptr));
    REFUSED(ou_overlap_add(nullptr, 8, 20, 8, 2, 0, 3, f.p, y, nullptr));
    REFUSED(ou_overlap_add(x, 8, 20, 8, 2, 0, 3, f.p, nullptr, nullptr));
    REFUSED(ou_overlap_add(x, 8, 20, 8, 2, 0, 3, nullptr, y, nullptr));          // O > 0 needs the table
    REFUSED(ou_overlap_add(x, 8, 20, 8, 2, 0, 0, f.p, y, nullptr));              // count
    REFUSED(ou_overlap_add(x, 8, 20, 8, 2, 0, -2, f.p, y, nullptr));
    REFUSED(ou_overlap_add(x, 7, 20, 8, 2, 0, 3, f.p, y, nullptr));              // windows overlap in w
    REFUSED(ou_overlap_add(x, 8, 20, 0, 0, 0, 3, f.p, y, nullptr));              // window
    REFUSED(ou_overlap_add(x, 8, 20, 8, 5, 0, 3, f.p, y, nullptr));              // O > W / 2
    REFUSED(ou_overlap_add(x, 8, 20, 8, -1, 0, 3, f.p, y, nullptr));
    REFUSED(ou_overlap_add(x, 8, 0, 8, 2, 0, 3, f.p, y, nullptr));               // T < 1
    REFUSED(ou_overlap_add(x, 8, 7, 8, 2, 0, 3, f.p, y, nullptr));               // T < W
    REFUSED(ou_overlap_add(x, 8, 20, 8, 2, -1, 3, f.p, y, nullptr));             // first < 0
    REFUSED(ou_overlap_add(x, 8, 20, 8, 2, 3, 1, f.p, y, nullptr));              // a group past the end
    OK(ou_overlap_add(x, 8, 20, 8, 0, 0, 3, nullptr, y, nullptr));               // O = 0 needs no table

    REFUSED(ou_long_windows(20, 8, 5, nullptr, nullptr));
    REFUSED(ou_long_windows(7, 8, 2, nullptr, nullptr));
    REFUSED(ou_long_fade(-1, f.p));
    REFUSED(ou_long_fade(2, nullptr));
}

// T past 2^31: the arguments only -- nothing is allocated or launched (the
// pointers are never dereferenced: both calls are refused on `first`)
void run_past_2_31()
{
    const int64_t T = (1LL << 31) + 12345, W = 4000, O = 800, H = W - O;
    int64_t n = 0, last = 0;
    CHECK(ou_long_windows(T, (int)W, (int)O, &n, &last) == 0, "%s", ouhip_detail::err_buf());
    CHECK(n == 1 + (T - W + H - 1) / H && n > 671000, "n %lld", (long long)n);
    CHECK(last == T - W && last > (1LL << 31), "last start %lld", (long long)last);
    LongGeom g;
    CHECK(long_geom("t", T, (int)W, (int)O, &g) == 0, "geometry");
    CHECK(win_start(g, n - 2) == (n - 2) * H && win_start(g, n - 2) > (1LL << 31), "start %lld", win_start(g, n - 2));
    CHECK(win_start(g, n - 1) == T - W && win_start(g, n + 7) == T - W, "clamp");
    CHECK(win_start(g, n - 1) - win_start(g, n - 2) <= H, "gap");
    float dummy = 0.f;
    REFUSED(ou_window_gather(&dummy, 0, 1, T, (int)W, (int)O, n, 8, W, &dummy, 0, W, nullptr));
    REFUSED(ou_overlap_add(&dummy, W, T, (int)W, (int)O, n, 8, &dummy, &dummy, nullptr));
    REFUSED(ou_window_gather(&dummy, 0, 1, T, (int)W, (int)O, -1, 8, W, &dummy, 0, W, nullptr));
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
