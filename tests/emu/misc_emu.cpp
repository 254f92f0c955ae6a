// Bounds check of the small kernels (ou_misc.hip) on the CPU: the HIP source
// compiled for the host against tests/emu/hip/hip_runtime.h, under
// AddressSanitizer.  Every op runs over the case tables of
// tests/test_gpu_misc.py, ou_embed and ou_snake_aa also at exactly the
// largest sizes their entry points accept.  Every buffer is an exact-size
// heap block (strided inputs end with the last item's window), and the
// kernels' static __shared__ arrays are per-call stack arrays here, so any
// global or LDS access outside an array aborts with its location.  The
// values computed are meaningless (no barriers, LDS not shared).
//
// Then every entry point must refuse null pointers, non-positive sizes and
// the sizes just past what the LDS arrays hold.  -DOU_EMU_MISC_OVER compiles
// that section out and launches one over-limit descriptor instead (argv[1]:
// "embed" = n_rff 129): against a source that accepts it, AddressSanitizer
// reports the LDS overrun.  See tests/test_emu_kernels.py.
#ifdef OU_EMU_MISC_SRC   // a modified copy of the kernel source (tests/test_emu_kernels.py)
#include OU_EMU_MISC_SRC
#else
#include "../../open_universe_amd/csrc/ou_misc.hip"
#endif

#include <string>

namespace {

// the largest sizes the entry points accept (checked from both sides: these
// run in bounds below, one more is refused)
constexpr int kMaxRff = 128, kMaxDim = 1024, kMaxTapsUp = 32, kMaxTapsDown = 64;

struct Pool {
    std::vector<void*> own;
    float* f(size_t n, float v = 0.25f)
    {
        float* p = (float*)std::malloc((n ? n : 1) * sizeof(float));   // exact size: ASan guards both ends
        for (size_t i = 0; i < n; ++i) p[i] = v;
        own.push_back(p);
        return p;
    }
    ~Pool() { for (void* p : own) std::free(p); }
};

int g_launches = 0;

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

const int kLens[] = {1, 3, 4, 1023, 4099, 16391};

void run_reductions()
{
    const int B = 2;
    for (int n : kLens) {
        Pool p;
        float* x = p.f((size_t)B * n);
        float* y = p.f((size_t)B * n);
        float* o = p.f(B);
        OK(ou_normalize(x, y, B, n, 0.05f, 1e-5f, nullptr));
        OK(ou_rms(x, o, B, n, nullptr));
        OK(ou_inv_rms(x, o, B, n, 7.f, 1e-5f, nullptr));
    }
    for (int left : {0, 1, 2, 3, 5})
        for (int len : kLens)
            for (int rms = 0; rms < 2; ++rms) {
                Pool p;
                const int64_t bs = left + len + 7;
                float* x = p.f((size_t)((B - 1) * bs + left + len));   // ends with the last item's window
                float* y = p.f((size_t)B * len);
                float* m = p.f(B);
                OK(ou_finish(x, bs, left, y, B, len, rms ? m : nullptr, nullptr));
            }
}

void run_elementwise()
{
    const int B = 2;
    {
        Pool p;
        const int nf = 5, fr = 7;
        OK(ou_power(p.f((size_t)B * 2 * nf * fr), p.f((size_t)B * nf * fr), B, nf, fr, nullptr));
    }
    const int pads[][3] = {{5, 16, 0}, {5, 16, 4}, {5, 16, 11}, {300, 513, 100}};
    for (auto& c : pads) {
        Pool p;
        const int64_t bs = c[0] + 3;
        OK(ou_pad(p.f((size_t)((B - 1) * bs + c[0])), bs, p.f((size_t)B * c[1]), B, c[0], c[1], c[2], nullptr));
    }
    for (int n : {1, 255, 256, 257, 1000})
        for (int add = 0; add < 2; ++add) {
            Pool p;
            OK(ou_scale(p.f(n), p.f(n), n, 0.3f, add ? p.f(n) : nullptr, nullptr));
        }
}

// a valid descriptor over exact-size buffers
ou_embed_desc embed_desc(Pool& p, int kind, int n, int n_rff, int dim, int rows)
{
    ou_embed_desc d{};
    float* sigma = p.f(n);
    for (int i = 0; i < n; ++i) sigma[i] = 1e-4f * (float)std::pow(100.0, i);
    d.sigma = sigma; d.n = n; d.kind = kind; d.dim = dim; d.rows = rows;
    d.te_weight = 0.7f; d.te_bias = -0.2f;
    if (kind == 1) {
        d.rff_freq = p.f(n_rff); d.n_rff = n_rff;
        const int din[3] = {2 * n_rff, 4 * n_rff, 8 * n_rff}, dout[3] = {4 * n_rff, 8 * n_rff, dim};
        for (int l = 0; l < 3; ++l) {
            d.mlp_w[l] = p.f((size_t)dout[l] * din[l], 0.01f);
            d.mlp_b[l] = p.f(dout[l]);
            d.mlp_slope[l] = 0.1f * (l + 1);
        }
    }
    d.w = p.f((size_t)rows * dim); d.bias = p.f(rows);
    d.out = p.f((size_t)n * rows); d.gbuf = p.f((size_t)n * dim);
    return d;
}

void run_embed()
{
    for (int n : {1, 3}) {
        for (int dim : {64, 96, 512})
            for (int rows : {1, 6, 64}) {
                Pool p;
                ou_embed_desc d = embed_desc(p, 0, n, 0, dim, rows);
                OK(ou_embed(&d, nullptr));
            }
        const int sb[][2] = {{4, 40}, {32, 512}, {kMaxRff, kMaxDim}};
        for (auto& c : sb)
            for (int rows : {5, 64}) {
                Pool p;
                ou_embed_desc d = embed_desc(p, 1, n, c[0], c[1], rows);
                OK(ou_embed(&d, nullptr));
            }
    }
}

ou_head_desc head_desc(Pool& p, int C, int T, int B, int mode, int edm)
{
    ou_head_desc d{};
    d.h_bstride = (int64_t)C * T + 5;
    d.h = p.f((size_t)((B - 1) * d.h_bstride + (int64_t)C * T));
    d.channels = C; d.length = T; d.batch = B; d.mode = mode;
    d.slope1 = 0.25f; d.slope2 = 0.1f;
    d.w = p.f((size_t)C * 3); d.bias = 0.01f; d.edm = edm;
    d.w_skip = 0.5f; d.w_out = 0.4f; d.s2 = 0.25f; d.c_score = 0.1f; d.c_noise = 0.2f; d.s_next = 0.3f;
    if (mode != 0) d.x = p.f((size_t)B * T);
    if (mode == 1) d.z = p.f((size_t)B * T);
    d.out = p.f((size_t)B * T);
    return d;
}

void run_head()
{
    for (int C : {1, 4, 8, 12, 33})
        for (int T : {1, 2, 256, 257, 515})
            for (int mode = 0; mode < 3; ++mode)
                for (int edm = 0; edm < 2; ++edm) {
                    Pool p;
                    ou_head_desc d = head_desc(p, C, T, 2, mode, edm);
                    OK(ou_head(&d, nullptr));
                }
}

ou_snake_desc snake_desc(Pool& p, int C, int T, int B, int tu, int wu, int td, int wd)
{
    ou_snake_desc d{};
    d.h_bstride = (int64_t)C * T + 3;
    d.h = p.f((size_t)((B - 1) * d.h_bstride + (int64_t)C * T));
    d.channels = C; d.length = T; d.batch = B;
    d.alpha = p.f(C, 1.f);
    d.k_up = p.f((size_t)2 * tu, 0.1f); d.taps_up = tu; d.width_up = wu;
    d.k_down = p.f(td, 0.05f); d.taps_down = td; d.width_down = wd;
    d.out = p.f((size_t)B * C * T);
    return d;
}

void run_snake()
{
    // the shipped filters (dsp.sinc_resample_kernel(1, 2) / (2, 1)), the
    // longest accepted ones, and single taps
    const int filt[][4] = {{15, 7, 28, 13}, {kMaxTapsUp, 15, kMaxTapsDown, 31}, {kMaxTapsUp, 0, kMaxTapsDown, 0},
                           {1, 0, 1, 0}};
    for (auto& f : filt)
        for (int T : {1, 2, 13, 255, 256, 257, 700}) {
            Pool p;
            ou_snake_desc d = snake_desc(p, 3, T, 2, f[0], f[1], f[2], f[3]);
            OK(ou_snake_aa(&d, nullptr));
        }
}

#ifndef OU_EMU_MISC_OVER
int g_refusals = 0;

#define REFUSED(call)                                                                         \
    do {                                                                                      \
        if ((call) == 0) {                                                                    \
            std::fprintf(stderr, "%s:%d: %s was accepted\n", __FILE__, __LINE__, #call);      \
            std::exit(3);                                                                     \
        }                                                                                     \
        ++g_refusals;                                                                         \
    } while (0)

// descriptor entry points: the valid descriptor with one field changed
#define REFUSED_WITH(fn, base, edit)                                                          \
    do {                                                                                      \
        auto d = (base);                                                                      \
        edit;                                                                                 \
        REFUSED(fn(&d, nullptr));                                                             \
    } while (0)

void run_rejections()
{
    Pool p;
    float* a = p.f(64);
    float* b = p.f(64);
    float* c = p.f(64);
    REFUSED(ou_normalize(nullptr, b, 2, 8, 1.f, 1e-5f, nullptr));
    REFUSED(ou_normalize(a, nullptr, 2, 8, 1.f, 1e-5f, nullptr));
    REFUSED(ou_normalize(a, b, 0, 8, 1.f, 1e-5f, nullptr));
    REFUSED(ou_normalize(a, b, 2, 0, 1.f, 1e-5f, nullptr));
    REFUSED(ou_normalize(a, b, 2, -3, 1.f, 1e-5f, nullptr));
    REFUSED(ou_inv_rms(nullptr, b, 2, 8, 8.f, 1e-5f, nullptr));
    REFUSED(ou_inv_rms(a, nullptr, 2, 8, 8.f, 1e-5f, nullptr));
    REFUSED(ou_inv_rms(a, b, -1, 8, 8.f, 1e-5f, nullptr));
    REFUSED(ou_inv_rms(a, b, 2, 0, 8.f, 1e-5f, nullptr));
    REFUSED(ou_rms(nullptr, b, 2, 8, nullptr));
    REFUSED(ou_rms(a, nullptr, 2, 8, nullptr));
    REFUSED(ou_rms(a, b, 0, 8, nullptr));
    REFUSED(ou_rms(a, b, 2, 0, nullptr));
    REFUSED(ou_power(nullptr, b, 1, 2, 3, nullptr));
    REFUSED(ou_power(a, nullptr, 1, 2, 3, nullptr));
    REFUSED(ou_power(a, b, 0, 2, 3, nullptr));
    REFUSED(ou_power(a, b, 1, 0, 3, nullptr));
    REFUSED(ou_power(a, b, 1, 2, 0, nullptr));
    REFUSED(ou_power(a, b, 1, -2, -3, nullptr));   // a positive product of negative sizes
    REFUSED(ou_pad(nullptr, 8, b, 2, 5, 16, 0, nullptr));
    REFUSED(ou_pad(a, 8, nullptr, 2, 5, 16, 0, nullptr));
    REFUSED(ou_pad(a, 8, b, 0, 5, 16, 0, nullptr));
    REFUSED(ou_pad(a, 8, b, 2, 0, 16, 0, nullptr));
    REFUSED(ou_pad(a, 8, b, 2, 5, 0, 0, nullptr));
    REFUSED(ou_pad(a, 8, b, -2, 5, -16, 0, nullptr));
    REFUSED(ou_scale(nullptr, b, 8, 1.f, nullptr, nullptr));
    REFUSED(ou_scale(a, nullptr, 8, 1.f, nullptr, nullptr));
    REFUSED(ou_scale(a, b, 0, 1.f, nullptr, nullptr));
    REFUSED(ou_scale(a, b, -8, 1.f, c, nullptr));
    REFUSED(ou_finish(nullptr, 16, 1, b, 2, 8, nullptr, nullptr));
    REFUSED(ou_finish(a, 16, 1, nullptr, 2, 8, nullptr, nullptr));
    REFUSED(ou_finish(a, 16, 1, b, 0, 8, nullptr, nullptr));
    REFUSED(ou_finish(a, 16, 1, b, 2, 0, c, nullptr));

    REFUSED(ou_embed(nullptr, nullptr));
    for (int kind = 0; kind < 2; ++kind) {
        const ou_embed_desc e = embed_desc(p, kind, 2, 4, 40, 5);
        REFUSED_WITH(ou_embed, e, d.sigma = nullptr);
        REFUSED_WITH(ou_embed, e, d.out = nullptr);
        REFUSED_WITH(ou_embed, e, d.w = nullptr);
        REFUSED_WITH(ou_embed, e, d.bias = nullptr);
        REFUSED_WITH(ou_embed, e, d.gbuf = nullptr);
        REFUSED_WITH(ou_embed, e, d.n = 0);
        REFUSED_WITH(ou_embed, e, d.dim = 0);
        REFUSED_WITH(ou_embed, e, d.rows = 0);
        REFUSED_WITH(ou_embed, e, d.rows = -4);
    }
    {
        const ou_embed_desc e = embed_desc(p, 1, 2, 4, 40, 5);
        REFUSED_WITH(ou_embed, e, d.kind = 2);
        REFUSED_WITH(ou_embed, e, d.rff_freq = nullptr);
        REFUSED_WITH(ou_embed, e, d.n_rff = 0);
        for (int l = 0; l < 3; ++l) {
            REFUSED_WITH(ou_embed, e, d.mlp_w[l] = nullptr);
            REFUSED_WITH(ou_embed, e, d.mlp_b[l] = nullptr);
        }
        // one past what the LDS buffers hold (the buffers here are sized for
        // the over-limit descriptor, so only the LDS arrays would overflow)
        const ou_embed_desc big_rff = embed_desc(p, 1, 1, kMaxRff + 1, kMaxDim, 5);
        REFUSED(ou_embed(&big_rff, nullptr));
        const ou_embed_desc big_dim = embed_desc(p, 1, 1, kMaxRff, kMaxDim + 1, 5);
        REFUSED(ou_embed(&big_dim, nullptr));
    }

    REFUSED(ou_head(nullptr, nullptr));
    {
        const ou_head_desc h = head_desc(p, 4, 9, 2, 1, 1);
        REFUSED_WITH(ou_head, h, d.h = nullptr);
        REFUSED_WITH(ou_head, h, d.w = nullptr);
        REFUSED_WITH(ou_head, h, d.out = nullptr);
        REFUSED_WITH(ou_head, h, d.x = nullptr);
        REFUSED_WITH(ou_head, h, d.z = nullptr);
        REFUSED_WITH(ou_head, h, (d.mode = 2, d.x = nullptr));
        REFUSED_WITH(ou_head, h, d.channels = 0);
        REFUSED_WITH(ou_head, h, d.length = 0);
        REFUSED_WITH(ou_head, h, d.batch = 0);
        REFUSED_WITH(ou_head, h, d.batch = -1);
    }

    REFUSED(ou_snake_aa(nullptr, nullptr));
    {
        const ou_snake_desc s = snake_desc(p, 3, 13, 2, 15, 7, 28, 13);
        REFUSED_WITH(ou_snake_aa, s, d.h = nullptr);
        REFUSED_WITH(ou_snake_aa, s, d.out = nullptr);
        REFUSED_WITH(ou_snake_aa, s, d.alpha = nullptr);
        REFUSED_WITH(ou_snake_aa, s, d.k_up = nullptr);
        REFUSED_WITH(ou_snake_aa, s, d.k_down = nullptr);
        REFUSED_WITH(ou_snake_aa, s, d.length = 0);
        REFUSED_WITH(ou_snake_aa, s, d.channels = 0);
        REFUSED_WITH(ou_snake_aa, s, d.batch = 0);
        REFUSED_WITH(ou_snake_aa, s, d.taps_up = 0);
        REFUSED_WITH(ou_snake_aa, s, d.taps_down = 0);
        REFUSED_WITH(ou_snake_aa, s, d.taps_up = -1);
        // just outside the limit on either side (filters sized for them)
        const ou_snake_desc up = snake_desc(p, 3, 257, 2, kMaxTapsUp + 1, 16, kMaxTapsDown, 31);
        REFUSED(ou_snake_aa(&up, nullptr));
        const ou_snake_desc down = snake_desc(p, 3, 257, 2, kMaxTapsUp, 15, kMaxTapsDown + 1, 32);
        REFUSED(ou_snake_aa(&down, nullptr));
    }
}
#endif

}  // namespace

int main(int argc, char** argv)
{
#ifdef OU_EMU_MISC_OVER
    const std::string what = argc > 1 ? argv[1] : "";
    int rc = -1;
    if (what == "embed") {
        Pool p;
        const ou_embed_desc d = embed_desc(p, 1, 1, kMaxRff + 1, kMaxDim, 5);
        rc = ou_embed(&d, nullptr);
    } else {
        std::fprintf(stderr, "usage: %s embed\n", argv[0]);
        return 2;
    }
    std::printf(rc ? "refused: %s\n" : "ran in bounds: %s\n", what.c_str());
    return 0;
#else
    (void)argc, (void)argv;
    run_reductions();
    run_elementwise();
    run_embed();
    run_head();
    run_snake();
    run_rejections();
    std::printf("ok: %d launches bounds-checked, %d descriptors refused\n", g_launches, g_refusals);
    return 0;
#endif
}
