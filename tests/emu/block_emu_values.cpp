// Numerics of the fused ConvBlock kernel (ou_block.hip) on the CPU (fiber
// emulator, tests/emu/hip/hip_runtime.h with OU_EMU_FIBERS): each launch is
// compared with a double-precision evaluation of the ou_block_desc formula
// (include/ouhip.h, blocks.py:393-416), whole-signal and on a frame range
// (f0, f1, h0, h1: only the range is stored and compared).  Channel counts
// 32 / 48 / 64 / 96 / 128 / 192 (48: MFMA rows padded to 64), f32,
// split-f16 and f16 operands, the epilogues FiLM, input_cond + FiLM, cond_out and res2,
// and split images (ou_block_desc.xs: stage 0 copies the producer's image of
// the operand; .sy: the epilogue stores prelu(y) 2^-s for the next conv).
// The score network's ends (groups 6 and up, run_end below): the fused input
// conv kEpiIn (alone, with FiLM, with FiLM and the rate-change conv) and the
// fused head kEpiHead (alone, with input_cond + FiLM; every sampler mode, with
// and without the EDM wrapper, out written over x) at 32 and 48 channels,
// batch 2, at 1, 3, Fo + 1 and 2 Fo + 1 frames (Fo: the frames a workgroup of
// the variant owns).
// Prints one line per failing case and exits 1.
#ifdef OU_EMU_BLOCK_SRC   // a modified copy of the kernel source (tests/test_emu_kernels.py)
#include OU_EMU_BLOCK_SRC
#else
#include "../../open_universe_amd/csrc/ou_block.hip"
#endif

#include <cmath>
#include <string>

static uint32_t g_seed = 777;
static float rnd()
{
    g_seed = g_seed * 1664525u + 1013904223u;
    return ((g_seed >> 8) & 0xffff) / 32768.0f - 1.0f;
}

struct Case {
    int C, T, prec;
    bool film, sc, cond, res2, chunk;
    bool xs = false, sy = false;
};

// prelu_slope(v) 2^-shift as a split image [C / 32][rows][hi | lo][32] f16
static std::vector<_Float16> split_image(const std::vector<float>& v, int C, int T, int rows, float slope, int shift)
{
    std::vector<_Float16> img((size_t)C / 32 * rows * 64, (_Float16)0.f);
    for (int c = 0; c < C; ++c)
        for (int t = 0; t < T; ++t) {
            float p = std::ldexp(v[(size_t)c * T + t], -shift);
            if (p < 0) p *= slope;
            const _Float16 hi = (_Float16)p;
            const size_t o = ((size_t)(c / 32) * rows + t) * 64 + c % 32;
            img[o] = hi;
            img[o + 32] = (_Float16)((p - (float)hi) * 2048.f);
        }
    return img;
}

// conv over [0, T) with zero padding: out[m][t] = b[m] + sum w[m][c][k] prelu(in[c][t + k - pad])
static void conv_ref(const std::vector<double>& in, const std::vector<float>& w, const std::vector<float>& b, int C,
                     int T, int kt, double slope, std::vector<double>& out)
{
    const int pad = (kt - 1) / 2;
    out.assign((size_t)C * T, 0.0);
    for (int m = 0; m < C; ++m)
        for (int t = 0; t < T; ++t) {
            double acc = b[m];
            for (int c = 0; c < C; ++c)
                for (int k = 0; k < kt; ++k) {
                    const int u = t + k - pad;
                    if (u < 0 || u >= T) continue;
                    double v = in[(size_t)c * T + u];
                    if (v < 0) v *= slope;
                    acc += (double)w[((size_t)m * C + c) * kt + k] * v;
                }
            out[(size_t)m * T + t] = acc;
        }
}

static int run(const Case& cs)
{
    const int C = cs.C, T = cs.T;
    const int kts[3] = {5, 3, 3};
    const float slopes[3] = {0.25f, 0.1f, 0.3f};
    std::vector<float> w[3], bias[3];
    std::vector<std::vector<_Float16>> packed(3);
    std::vector<std::vector<float>> packed32(3);
    ou_block_desc d{};
    for (int i = 0; i < 3; ++i) {
        w[i].resize((size_t)C * C * kts[i]);
        for (auto& e : w[i]) e = rnd() / std::sqrt((float)(C * kts[i]));
        bias[i].resize(C);
        for (auto& e : bias[i]) e = 0.1f * rnd();
        if (cs.prec == 0) {
            packed32[i].resize(ou_block_packed_f32(C, kts[i]));
            if (ou_block_pack_f32(w[i].data(), C, kts[i], packed32[i].data(), &d.w_unscale[i]) != 0) return 10;
            d.w[i] = packed32[i].data();
        } else {
            packed[i].resize(ou_block_packed_halves(C, kts[i]));
            if (ou_block_pack(w[i].data(), C, kts[i], packed[i].data(), &d.w_unscale[i]) != 0) return 10;
            d.w[i] = packed[i].data();
        }
        d.bias[i] = bias[i].data();
        d.slope[i] = slopes[i];
    }
    std::vector<float> h((size_t)C * T), sc((size_t)C * T), film(2 * C), res2((size_t)C * T);
    for (auto* v : {&h, &sc, &film, &res2})
        for (auto& e : *v) e = rnd();
    for (int c = 0; c < C; ++c) film[c] = 1.0f + 0.2f * film[c];   // gamma near 1
    std::vector<float> y((size_t)C * T, 1e30f), co((size_t)C * T, 1e30f);
    int status = 0;
    d.h = h.data(); d.h_bstride = (int64_t)C * T; d.h_cstride = T;
    d.channels = C; d.length = T; d.batch = 1; d.prec = cs.prec;
    if (cs.sc) { d.sc = sc.data(); d.sc_bstride = (int64_t)C * T; d.sc_cstride = T; d.s_sc = 0.7f; }
    if (cs.film) { d.film = film.data(); d.film_bstride = 2 * C; }
    if (cs.cond) { d.cond_out = co.data(); d.co_bstride = (int64_t)C * T; d.co_cstride = T; }
    d.y = y.data(); d.y_bstride = (int64_t)C * T; d.y_cstride = T; d.s_res = 0.7f; d.s2 = 0.5f;
    if (cs.res2) { d.res2 = res2.data(); d.r2_bstride = (int64_t)C * T; d.r2_cstride = T; }
    d.status = &status;
    d.shift[0] = 7; d.shift[1] = 5; d.shift[2] = 6; d.shift[3] = 6;
    const int rows = T + 3, sshift = 9;
    const float sslope = 0.125f;
    std::vector<_Float16> ximg, yimg((size_t)C / 32 * rows * 64, (_Float16)1e4f);
    if (cs.xs) {
        ximg = split_image(h, C, T, rows, slopes[0], d.shift[0]);
        d.xs = (const uint16_t*)ximg.data(); d.xs_bstride = (int64_t)ximg.size() * 2; d.xs_rows = rows;
    }
    if (cs.sy) {
        d.sy = (uint16_t*)yimg.data(); d.sy_bstride = (int64_t)yimg.size() * 2; d.sy_rows = rows;
        d.sy_shift = sshift; d.sy_slope = sslope;
    }
    int f0 = 0, f1 = T;
    if (cs.chunk) {
        f0 = T / 3;
        f1 = 2 * T / 3 + 1;
        d.f0 = f0; d.f1 = f1;
        d.h0 = std::max(0, f0 - 4); d.h1 = std::min(T, f1 + 4);   // exactly what [f0, f1) reads
        for (int c = 0; c < C; ++c)   // h outside [h0, h1) is garbage the kernel must not read
            for (int t = 0; t < T; ++t)
                if (t < d.h0 || t >= d.h1) h[(size_t)c * T + t] = 1e30f;
    }
    // reference (h outside [h0, h1) is not needed by [f0, f1))
    std::vector<double> hd((size_t)C * T), c1, c2, c3;
    for (size_t i = 0; i < hd.size(); ++i) hd[i] = h[i] == 1e30f ? 0.0 : h[i];
    conv_ref(hd, w[0], bias[0], C, T, 5, slopes[0], c1);
    for (int m = 0; m < C; ++m)
        for (int t = 0; t < T; ++t) {
            double& v = c1[(size_t)m * T + t];
            if (cs.sc) v = (v + sc[(size_t)m * T + t]) * 0.7;
            if (cs.film) v = film[m] * v + film[C + m];
        }
    conv_ref(c1, w[1], bias[1], C, T, 3, slopes[1], c2);
    conv_ref(c2, w[2], bias[2], C, T, 3, slopes[2], c3);
    const int rc = ou_block(&d, nullptr);
    if (rc != 0) {
        std::printf("C %d T %d prec %d: launch error %d: %s\n", C, T, cs.prec, rc, ouhip_detail::err_buf());
        return 1;
    }
    double en = 0, rn = 0, ec = 0, rc2 = 0;
    bool outside = false;
    for (int m = 0; m < C; ++m)
        for (int t = 0; t < T; ++t) {
            const size_t o = (size_t)m * T + t;
            if (t < f0 || t >= f1) {
                outside |= y[o] != 1e30f || (cs.cond && co[o] != 1e30f);
                continue;
            }
            double want = (hd[o] + c3[o]) * 0.7;
            if (cs.res2) want = (want + res2[o]) * 0.5;
            en += (y[o] - want) * (y[o] - want);
            rn += want * want;
            if (cs.cond) {
                ec += (co[o] - c1[o]) * (co[o] - c1[o]);
                rc2 += c1[o] * c1[o];
            }
        }
    bool img_bad = false;   // the stored split image: prelu(y) 2^-s element by element, rows >= T untouched
    if (cs.sy)
        for (int c = 0; c < C; ++c)
            for (int t = 0; t < rows; ++t) {
                const size_t o = ((size_t)(c / 32) * rows + t) * 64 + c % 32;
                if (t >= T) {
                    img_bad |= (float)yimg[o] != 1e4f || (float)yimg[o + 32] != 1e4f;
                    continue;
                }
                double p = std::ldexp((double)y[(size_t)c * T + t], -sshift);
                if (p < 0) p *= sslope;
                const double got = (double)yimg[o] + (double)yimg[o + 32] / 2048.0;
                img_bad |= !(std::fabs(got - p) <= std::fabs(p) * std::ldexp(1.0, -21) + std::ldexp(1.0, -35));
            }
    const double rel = std::sqrt(en / rn), relc = cs.cond ? std::sqrt(ec / rc2) : 0.0;
    const double tol = cs.prec == 2 ? 3e-3 : 2e-5;
    if (!(rel < tol) || !(relc < tol) || outside || status || img_bad) {
        std::printf("C %d T %d prec %d film %d sc %d cond %d res2 %d chunk %d xs %d sy %d: rel %.3g cond %.3g "
                    "outside %d status %d image %d\n",
                    C, T, cs.prec, cs.film, cs.sc, cs.cond, cs.res2, cs.chunk, cs.xs, cs.sy, rel, relc, outside,
                    status, img_bad);
        return 1;
    }
    return 0;
}

// ---- the score network's ends: kEpiIn (+ FiLM, + kEpiDown) and kEpiHead
struct EndCase {
    int C, T, prec;
    bool film;
    bool in, scale;   // kEpiIn: h = input_conv(in_scale[b] x); scale: per-item in_scale, else NULL
    int kt;           // with kEpiIn: the rate-2 rate-change conv of down_kt frames (0: none)
    bool sc, head;    // kEpiHead; sc: input_cond on conv1 (the decoder form)
    int mode, edm;
    bool neg;         // head slopes (-0.5, 0.1): the order of the two PReLUs shows
};

static const float kPoison = 1e30f;

static bool all_poison(const std::vector<float>& v, size_t a, size_t b)
{
    for (size_t i = a; i < b; ++i)
        if (v[i] != kPoison) return false;
    return true;
}

// owned frames of a workgroup of the variant (block_f of the kernel)
static int end_frames(const EndCase& cs)
{
    const int F = ou_block_frames(cs.C);
    if (cs.head) return F - 2;
    if (cs.kt) return (F - 2 * 2 * ((cs.kt - 1) / 2)) / 2 * 2;
    return F;
}

static int run_end(const EndCase& cs, double* worst)
{
    const int C = cs.C, T = cs.T, B = 2, R = 2;
    const int kts[3] = {5, 3, 3};
    const float slopes[3] = {0.25f, 0.1f, 0.3f};
    std::vector<float> w[3], bias[3];
    std::vector<std::vector<_Float16>> packed(3);
    std::vector<std::vector<float>> packed32(3);
    ou_block_desc d{};
    for (int i = 0; i < 3; ++i) {
        w[i].resize((size_t)C * C * kts[i]);
        for (auto& e : w[i]) e = rnd() / std::sqrt((float)(C * kts[i]));
        bias[i].resize(C);
        for (auto& e : bias[i]) e = 0.1f * rnd();
        if (cs.prec == 0) {
            packed32[i].resize(ou_block_packed_f32(C, kts[i]));
            if (ou_block_pack_f32(w[i].data(), C, kts[i], packed32[i].data(), &d.w_unscale[i]) != 0) return 10;
            d.w[i] = packed32[i].data();
        } else {
            packed[i].resize(ou_block_packed_halves(C, kts[i]));
            if (ou_block_pack(w[i].data(), C, kts[i], packed[i].data(), &d.w_unscale[i]) != 0) return 10;
            d.w[i] = packed[i].data();
        }
        d.bias[i] = bias[i].data();
        d.slope[i] = slopes[i];
    }
    const size_t CT = (size_t)C * T;
    // the block input: computed from x (rows T + 3 apart, poison between; +-50
    // at the clip's ends; h itself is poison the kernel must not read), or h
    const int xbs = T + 3;
    std::vector<float> x((size_t)B * xbs, kPoison), w_in(3 * C), b_in(C), h(B * CT);
    const float scales[2] = {0.5f, 2.0f};
    std::vector<double> hd(B * CT);
    if (cs.in) {
        for (auto& e : w_in) e = rnd();
        for (auto& e : b_in) e = 1.0f + rnd();   // order 1: h = b_in outside the clip would show
        for (int b = 0; b < B; ++b) {
            for (int t = 0; t < T; ++t) x[(size_t)b * xbs + t] = rnd();
            x[(size_t)b * xbs] = b ? -50.f : 50.f;
            x[(size_t)b * xbs + T - 1] = b ? 50.f : -50.f;
        }
        for (auto& e : h) e = kPoison;
        for (int b = 0; b < B; ++b)
            for (int c = 0; c < C; ++c)
                for (int t = 0; t < T; ++t) {
                    double acc = b_in[c];
                    for (int k = 0; k < 3; ++k) {
                        const int u = t + k - 1;
                        if (u < 0 || u >= T) continue;
                        acc += (double)w_in[3 * c + k] * ((cs.scale ? (double)scales[b] : 1.0) * x[(size_t)b * xbs + u]);
                    }
                    hd[b * CT + (size_t)c * T + t] = acc;
                }
        d.x = x.data(); d.x_bstride = xbs; d.in_scale = cs.scale ? scales : nullptr;
        d.w_in = w_in.data(); d.b_in = b_in.data();
    } else {
        for (auto& e : h) e = rnd();
        for (int b = 0; b < B; ++b)
            for (int c = 0; c < C; ++c) {
                const float s = (b + c) % 2 ? -50.f : 50.f;
                h[b * CT + (size_t)c * T] = s;
                h[b * CT + (size_t)c * T + T - 1] = -s;
            }
        for (size_t i = 0; i < hd.size(); ++i) hd[i] = h[i];
    }
    std::vector<float> sc(B * CT), film((size_t)B * 2 * C);
    for (auto& e : sc) e = rnd();
    for (auto& e : film) e = rnd();
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < C; ++c) film[(size_t)b * 2 * C + c] = 1.0f + 0.2f * film[(size_t)b * 2 * C + c];
    // outputs with a poison margin: rows 2 floats longer than T, one spare item
    const int ycs = T + 2, TE = (T + R - 1) / R, ecs = TE + 2;
    std::vector<float> y((size_t)(B + 1) * C * ycs, kPoison), e((size_t)(B + 1) * 2 * C * ecs, kPoison);
    int status = 0;
    d.h = h.data(); d.h_bstride = (int64_t)CT; d.h_cstride = T;
    d.channels = C; d.length = T; d.batch = B; d.prec = cs.prec;
    if (cs.sc) { d.sc = sc.data(); d.sc_bstride = (int64_t)CT; d.sc_cstride = T; d.s_sc = 0.7f; }
    if (cs.film) { d.film = film.data(); d.film_bstride = 2 * C; }
    d.y = y.data(); d.y_bstride = (int64_t)C * ycs; d.y_cstride = ycs; d.s_res = 0.7f; d.s2 = 1.f;
    d.status = &status;
    d.shift[0] = 7; d.shift[1] = 5; d.shift[2] = 6; d.shift[3] = 8;
    // the rate-change conv: w[2C][C][kt R] tap-major, e[m][u] over samples u R - R (kt - 1) / 2 + j
    const int KT = cs.kt * R;
    const float slope_down = 0.15f;
    std::vector<float> wd((size_t)2 * C * C * (KT ? KT : 1)), bd(2 * C);
    std::vector<_Float16> wdp;
    if (cs.kt) {
        for (auto& v : wd) v = rnd() / std::sqrt((float)(C * KT));
        for (auto& v : bd) v = 0.1f * rnd();
        wdp.resize((size_t)2 * C * C * KT * 2);
        if (ou_block_pack_rect(wd.data(), 2 * C, C, KT, wdp.data(), &d.w_down_unscale) != 0) return 10;
        d.w_down = wdp.data(); d.b_down = bd.data(); d.slope_down = slope_down; d.rate = R; d.down_kt = cs.kt;
        d.e = e.data(); d.e_bstride = (int64_t)2 * C * ecs; d.e_cstride = ecs;
    }
    // the head: sampler state xh (out written over it in modes 1 and 2), noise z
    const float s1 = cs.neg ? -0.5f : 0.25f, s2h = 0.1f;
    std::vector<float> hw(3 * C), xh((size_t)(B + 1) * T, kPoison), z((size_t)B * T), ho((size_t)(B + 1) * T, kPoison);
    for (auto& v : hw) v = rnd() / std::sqrt(3.f * C);
    for (int i = 0; i < B * T; ++i) xh[i] = rnd(), z[i] = rnd();
    const std::vector<float> xh0 = xh;
    float* out = cs.mode ? xh.data() : ho.data();
    if (cs.head) {
        ou_head_desc& q = d.head;
        q.channels = C; q.length = T; q.batch = B; q.mode = cs.mode;
        q.slope1 = s1; q.slope2 = s2h; q.w = hw.data(); q.bias = 0.05f; q.edm = cs.edm;
        q.w_skip = 0.8f; q.w_out = 0.6f; q.s2 = 0.49f; q.c_score = 0.3f; q.c_noise = 0.2f; q.s_next = 0.5f;
        q.x = cs.mode ? xh.data() : nullptr; q.z = cs.mode == 1 ? z.data() : nullptr; q.out = out;
    }
    const int rc = ou_block(&d, nullptr);
    std::string name = "end C " + std::to_string(C) + " T " + std::to_string(T) + " prec " + std::to_string(cs.prec) +
                       " film " + std::to_string(cs.film) + " in " + std::to_string(cs.in) + " scale " +
                       std::to_string(cs.scale) + " down_kt " + std::to_string(cs.kt) + " sc " + std::to_string(cs.sc) +
                       " head " + std::to_string(cs.head) + " mode " + std::to_string(cs.mode) + " edm " +
                       std::to_string(cs.edm) + " neg " + std::to_string(cs.neg);
    if (rc != 0) {
        std::printf("%s: launch error %d: %s\n", name.c_str(), rc, ouhip_detail::err_buf());
        return 1;
    }
    // reference, item by item
    double en = 0, rn = 0, ee = 0, re = 0, eh = 0, rh = 0, mx = 0;
    bool outside = false;
    const double kq = cs.mode == 0 ? 1.0 : cs.edm ? 0.3f * (double)0.6f / 0.49f : 0.3f;   // d out / d net
    for (int b = 0; b < B; ++b) {
        std::vector<double> hb(hd.begin() + b * CT, hd.begin() + (b + 1) * CT), c1, c2, c3, yr(CT);
        conv_ref(hb, w[0], bias[0], C, T, 5, slopes[0], c1);
        for (int m = 0; m < C; ++m)
            for (int t = 0; t < T; ++t) {
                double& v = c1[(size_t)m * T + t];
                if (cs.sc) v = (v + sc[b * CT + (size_t)m * T + t]) * 0.7f;
                if (cs.film) v = film[(size_t)b * 2 * C + m] * v + film[(size_t)b * 2 * C + C + m];
            }
        conv_ref(c1, w[1], bias[1], C, T, 3, slopes[1], c2);
        conv_ref(c2, w[2], bias[2], C, T, 3, slopes[2], c3);
        for (size_t i = 0; i < CT; ++i) yr[i] = (hb[i] + c3[i]) * 0.7f;
        if (cs.head) {
            for (int t = 0; t < T; ++t) {
                double net = 0.05f;
                for (int c = 0; c < C; ++c)
                    for (int k = 0; k < 3; ++k) {
                        const int u = t + k - 1;
                        if (u < 0 || u >= T) continue;
                        double v = yr[(size_t)c * T + u];
                        if (v < 0) v *= s1;
                        if (v < 0) v *= s2h;
                        net += (double)hw[3 * c + k] * v;
                    }
                double want = net;
                if (cs.mode) {
                    const double xv = xh0[(size_t)b * T + t];
                    const double score = cs.edm ? ((0.8f * xv + 0.6f * net) - xv) / 0.49f : net;
                    want = xv + 0.3f * score;
                    if (cs.mode == 1) want += 0.2f * ((double)z[(size_t)b * T + t] * 0.5f);
                }
                const double got = out[(size_t)b * T + t];
                eh += (got - want) * (got - want);
                rh += kq * net * kq * net;
                mx = std::fmax(mx, std::fabs(want));
            }
            continue;
        }
        for (int m = 0; m < C; ++m)
            for (int t = 0; t < T; ++t) {
                const double got = y[((size_t)b * C + m) * ycs + t], want = yr[(size_t)m * T + t];
                en += (got - want) * (got - want);
                rn += want * want;
            }
        for (int m = 0; m < C; ++m) outside |= !all_poison(y, ((size_t)b * C + m) * ycs + T, ((size_t)b * C + m + 1) * ycs);
        if (!cs.kt) continue;
        for (int m = 0; m < 2 * C; ++m) {
            for (int u = 0; u < TE; ++u) {
                double acc = bd[m];
                for (int c = 0; c < C; ++c)
                    for (int j = 0; j < KT; ++j) {
                        const int t = u * R - R * ((cs.kt - 1) / 2) + j;
                        if (t < 0 || t >= T) continue;
                        double v = yr[(size_t)c * T + t];
                        if (v < 0) v *= slope_down;
                        acc += (double)wd[((size_t)m * C + c) * KT + j] * v;
                    }
                const double got = e[((size_t)b * 2 * C + m) * ecs + u];
                ee += (got - acc) * (got - acc);
                re += acc * acc;
            }
            outside |= !all_poison(e, ((size_t)b * 2 * C + m) * ecs + TE, ((size_t)b * 2 * C + m + 1) * ecs);
        }
    }
    // nothing outside the windows: the spare item, every y of a head launch, e without the stage, x and out
    outside |= !all_poison(y, cs.head ? 0 : (size_t)B * C * ycs, y.size());
    outside |= !all_poison(e, cs.kt ? (size_t)B * 2 * C * ecs : 0, e.size());
    outside |= !all_poison(xh, (size_t)B * T, xh.size()) || !all_poison(ho, cs.head && !cs.mode ? (size_t)B * T : 0, ho.size());
    if (!cs.head || !cs.mode)
        for (int i = 0; i < B * T; ++i) outside |= xh[i] != xh0[i];
    const double tol = cs.prec == 2 ? 3e-3 : 2e-5;
    const double rel = cs.head ? 0.0 : std::sqrt(en / rn), rele = cs.kt ? std::sqrt(ee / re) : 0.0;
    // head: rms(out - ref) against rms(k net), k = d out / d net, so that the O(1) x term of the sampler
    // modes hides nothing; plus one f32 ulp of max |ref|
    const double n = (double)B * T;
    const double relh = cs.head ? std::sqrt(eh / rh) : 0.0;
    const bool head_ok = !cs.head || std::sqrt(eh / n) <= tol * std::sqrt(rh / n) + std::ldexp(mx, -23);
    worst[0] = std::fmax(worst[0], rel), worst[1] = std::fmax(worst[1], rele), worst[2] = std::fmax(worst[2], relh);
    if (!(rel < tol) || !(rele < tol) || !head_ok || outside || status) {
        std::printf("%s: rel %.3g e %.3g head %.3g outside %d status %d\n", name.c_str(), rel, rele, relh, outside,
                    status);
        return 1;
    }
    return 0;
}

static int run_ends(int group)
{
    int bad = 0, n = 0, g = 0;
    for (int C : {32, 48})
        for (int prec : {0, 1, 2}) {
            if (group >= 0 && g++ != group) continue;
            double worst[3] = {0, 0, 0};
            std::vector<EndCase> base;
            for (bool scale : {true, false}) {
                base.push_back({C, 0, prec, false, true, scale, 0, false, false, 0, 0, false});
                base.push_back({C, 0, prec, true, true, scale, 0, false, false, 0, 0, false});
                if (C == 32 && prec != 0)
                    for (int kt : {3, 1}) base.push_back({C, 0, prec, true, true, scale, kt, false, false, 0, 0, false});
            }
            for (int mode : {0, 1, 2})
                for (int edm : {0, 1})
                    for (bool neg : {false, true}) {
                        base.push_back({C, 0, prec, false, false, false, 0, false, true, mode, edm, neg});
                        base.push_back({C, 0, prec, true, false, false, 0, true, true, mode, edm, neg});
                    }
            for (EndCase cs : base) {
                const int Fo = end_frames(cs);
                for (int T : {1, 3, Fo + 1, 2 * Fo + 1}) {
                    cs.T = T;
                    bad += run_end(cs, worst);
                    ++n;
                }
            }
            std::printf("ends C %d prec %d: worst rel y %.3g e %.3g head %.3g\n", C, prec, worst[0], worst[1], worst[2]);
        }
    std::printf("%s: %d end-block launches checked, %d bad\n", bad ? "FAIL" : "ok", n, bad);
    return bad ? 1 : 0;
}

int main(int argc, char** argv)
{
    if (argc > 1 && std::atoi(argv[1]) >= 6) return run_ends(std::atoi(argv[1]) - 6);   // groups 6 ..: (C, prec) of the ends
    std::vector<Case> cases;
    for (int C : {48, 96, 192, 32, 64, 128})
        for (int prec : {0, 1, 2}) {
            const int T = C >= 128 ? 45 : 70;
            cases.push_back({C, T, prec, false, false, false, false, false});
            cases.push_back({C, T, prec, true, true, false, false, false});
            cases.push_back({C, T, prec, false, false, true, false, true});
            cases.push_back({C, T, prec, false, false, false, true, true});
            const bool img = prec == 1 && C % 32 == 0;   // split images: both ends, then input only
            cases.push_back({C, T, prec, true, true, false, false, false, img, img});
            cases.push_back({C, T, prec, false, false, true, false, false, img, false});
        }
    const int only = argc > 1 ? std::atoi(argv[1]) : -1;
    int bad = 0, n = 0;
    for (int i = 0; i < (int)cases.size(); ++i) {
        if (only >= 0 && i / 18 != only) continue;   // argv: channel-count group (18 cases each)
        bad += run(cases[i]);
        ++n;
    }
    std::printf("%s: %d block launches checked, %d bad\n", bad ? "FAIL" : "ok", n, bad);
    if (only < 0) bad += run_ends(-1);   // no argument: everything
    return bad ? 1 : 0;
}
