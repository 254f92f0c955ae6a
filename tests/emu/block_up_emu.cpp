// ou_block's fused up-sampling stage (kEpiUp, ou_block.hip) on the CPU: the
// HIP source compiled for the host against tests/emu/hip/hip_runtime.h in
// fiber mode (OU_EMU_FIBERS: barriers and the wave-wide MFMA are real) under
// AddressSanitizer.  Every kEpiUp instantiation the dispatcher has -- 64
// channels at rate 2 and 128 at rate 4, split-f16 and f16, plain / FiLM /
// input_cond + FiLM -- at lengths of several windows with a ragged last one,
// exactly one window and a signal shorter than the halo.  Every buffer is an
// exact-size heap block (any out-of-bounds global or LDS access aborts with
// its location), and u is compared with a double-precision evaluation of the
// ou_block_desc formula (include/ouhip.h): the block, PReLU, transposed
// conv, FIR 'same' with zeros outside, bias, zero from u_valid on, residual.
// Variants per case: the residual aliasing u (in place) or a buffer of its own
// or none, y stored or NULL, a cropped u_len, no FIR (up_taps NULL).
// See tests/test_emu_block_up.py.
#include "../../open_universe_amd/csrc/ou_block.hip"

#include <cmath>

static uint32_t g_seed = 4242;
static float rnd()
{
    g_seed = g_seed * 1664525u + 1013904223u;
    return ((g_seed >> 8) & 0xffff) / 32768.0f - 1.0f;
}

static float* alloc(size_t n)   // exact size: ASan guards both ends
{
    float* p = (float*)std::malloc((n ? n : 1) * sizeof(float));
    for (size_t i = 0; i < n; ++i) p[i] = rnd();
    return p;
}

// out[m][t] = b[m] + sum w[m][c][k] prelu(in[c][t + k - pad]) over [0, T), zero padding
static void conv_ref(const std::vector<double>& in, const std::vector<float>& w, const float* b, int C, int T, int kt,
                     double slope, std::vector<double>& out)
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

struct Case {
    int C, R, T, prec;
    bool film, sc;
    int res;      // 0 none, 1 in place (u_res == u), 2 its own buffer
    bool store_y, crop, fir;
};

static int run(const Case& cs)
{
    const int C = cs.C, R = cs.R, T = cs.T, CO = C / 2, CPT = 32 / R;
    const int kts[3] = {5, 3, 3};
    const float slopes[3] = {0.25f, 0.1f, 0.3f};
    const float slope_up = 0.2f;
    std::vector<void*> own;
    auto f = [&](size_t n) { float* p = alloc(n); own.push_back(p); return p; };
    ou_block_desc d{};
    std::vector<float> w[3];
    for (int i = 0; i < 3; ++i) {
        w[i].resize((size_t)C * C * kts[i]);
        for (auto& e : w[i]) e = rnd() / std::sqrt((float)(C * kts[i]));
        void* pk = std::malloc((size_t)ou_block_packed_halves(C, kts[i]) * sizeof(_Float16));
        own.push_back(pk);
        if (ou_block_pack(w[i].data(), C, kts[i], pk, &d.w_unscale[i]) != 0) return 10;
        d.w[i] = pk;
        float* b = f(C);
        for (int c = 0; c < C; ++c) b[c] *= 0.1f;
        d.bias[i] = b;
        d.slope[i] = slopes[i];
    }
    // transposed conv wt[ci][co][ph] -> rows 32 (co / CPT) + (co % CPT) R + ph of ou_block_pack_rect
    std::vector<float> wt((size_t)C * CO * R), wu((size_t)R * CO * C);
    for (auto& e : wt) e = rnd() / std::sqrt((float)C);
    for (int ci = 0; ci < C; ++ci)
        for (int co = 0; co < CO; ++co)
            for (int ph = 0; ph < R; ++ph)
                wu[(size_t)(32 * (co / CPT) + (co % CPT) * R + ph) * C + ci] = wt[((size_t)ci * CO + co) * R + ph];
    void* wup = std::malloc((size_t)R * CO * C * 2 * sizeof(_Float16));
    own.push_back(wup);
    if (ou_block_pack_rect(wu.data(), R * CO, C, 1, wup, &d.w_up_unscale) != 0) return 10;
    float* taps = f(2 * R + 1);
    double tsum = 0;
    for (int j = 0; j <= 2 * R; ++j) taps[j] = 1.f + 0.5f * taps[j], tsum += taps[j];
    for (int j = 0; j <= 2 * R; ++j) taps[j] = (float)(taps[j] * R / tsum);
    float* b_up = f(CO);

    float* h = f((size_t)C * T);
    float* sc = f((size_t)C * T);
    float* film = f(2 * C);
    for (int c = 0; c < C; ++c) film[c] = 1.0f + 0.2f * film[c];
    const int ulen = R * T - (cs.crop ? 1 : 0), uvalid = cs.crop ? ulen - 2 : R * T;
    float* u = f((size_t)CO * ulen);
    float* ures = cs.res == 2 ? f((size_t)CO * ulen) : cs.res == 1 ? u : nullptr;
    std::vector<float> res0(cs.res ? (size_t)CO * ulen : 0);
    for (size_t i = 0; i < res0.size(); ++i) res0[i] = ures[i];
    float* y = cs.store_y ? f((size_t)C * T) : nullptr;
    int* status = (int*)std::malloc(sizeof(int));
    own.push_back(status);
    *status = 0;
    d.h = h; d.h_bstride = (int64_t)C * T; d.h_cstride = T;
    d.channels = C; d.length = T; d.batch = 1; d.prec = cs.prec;
    if (cs.sc) { d.sc = sc; d.sc_bstride = (int64_t)C * T; d.sc_cstride = T; d.s_sc = 0.7f; }
    if (cs.film) { d.film = film; d.film_bstride = 2 * C; }
    d.y = y; d.y_bstride = (int64_t)C * T; d.y_cstride = T; d.s_res = 0.7f; d.s2 = 1.f;
    d.status = status;
    d.shift[0] = 7; d.shift[1] = 5; d.shift[2] = 6; d.shift[3] = 5;
    d.w_up = wup; d.b_up = b_up; d.up_taps = cs.fir ? taps : nullptr;
    d.slope_up = slope_up; d.up_rate = R;
    d.u = u; d.u_bstride = (int64_t)CO * ulen; d.u_cstride = ulen; d.u_len = ulen; d.u_valid = uvalid;
    d.u_res = ures; d.ur_bstride = (int64_t)CO * ulen; d.ur_cstride = ulen; d.s_u = 0.6f;

    std::vector<double> hd((size_t)C * T), c1, c2, c3;
    for (size_t i = 0; i < hd.size(); ++i) hd[i] = h[i];
    conv_ref(hd, w[0], d.bias[0], C, T, 5, slopes[0], c1);
    for (int m = 0; m < C; ++m)
        for (int t = 0; t < T; ++t) {
            double& v = c1[(size_t)m * T + t];
            if (cs.sc) v = (v + sc[(size_t)m * T + t]) * 0.7;
            if (cs.film) v = film[m] * v + film[C + m];
        }
    conv_ref(c1, w[1], d.bias[1], C, T, 3, slopes[1], c2);
    conv_ref(c2, w[2], d.bias[2], C, T, 3, slopes[2], c3);
    std::vector<double> yd((size_t)C * T), z((size_t)CO * R * T, 0.0);
    for (size_t i = 0; i < yd.size(); ++i) yd[i] = (hd[i] + c3[i]) * 0.7;
    for (int co = 0; co < CO; ++co)
        for (int t = 0; t < T; ++t)
            for (int ph = 0; ph < R; ++ph) {
                double acc = 0;
                for (int ci = 0; ci < C; ++ci) {
                    double v = yd[(size_t)ci * T + t];
                    if (v < 0) v *= slope_up;
                    acc += (double)wt[((size_t)ci * CO + co) * R + ph] * v;
                }
                z[(size_t)co * R * T + t * R + ph] = acc;
            }

    const int rc = ou_block(&d, nullptr);
    int bad = 0;
    if (rc != 0) {
        std::printf("launch error %d: %s\n", rc, ouhip_detail::err_buf());
        bad = 1;
    }
    double en = 0, rn = 0, ey = 0, ry = 0;
    for (int co = 0; co < CO && !bad; ++co)
        for (int s = 0; s < ulen; ++s) {
            double v = 0;
            if (cs.fir) {
                for (int j = 0; j <= 2 * R; ++j) {
                    const int q = s - R + j;
                    if (q >= 0 && q < R * T) v += (double)taps[j] * z[(size_t)co * R * T + q];
                }
            } else {
                v = z[(size_t)co * R * T + s];
            }
            v += b_up[co];
            if (s >= uvalid) v = 0;
            if (cs.res) v += res0[(size_t)co * ulen + s];
            v *= 0.6;
            const double got = u[(size_t)co * ulen + s];
            en += (got - v) * (got - v);
            rn += v * v;
        }
    if (y && !bad)
        for (size_t i = 0; i < yd.size(); ++i) ey += (y[i] - yd[i]) * (y[i] - yd[i]), ry += yd[i] * yd[i];
    const double rel = std::sqrt(en / rn), rely = y ? std::sqrt(ey / ry) : 0.0;
    const double tol = cs.prec == 2 ? 3e-3 : 2e-5;
    if (!bad && (!(rel < tol) || !(rely < tol) || *status)) bad = 1;
    if (bad || std::getenv("OUHIP_EMU_VERBOSE"))
        std::printf("C %d R %d T %d prec %d film %d sc %d res %d y %d crop %d fir %d: rel %.3g y %.3g status %d%s\n", C, R,
                    T, cs.prec, cs.film, cs.sc, cs.res, cs.store_y, cs.crop, cs.fir, rel, rely, *status,
                    bad ? "  FAIL" : "");
    for (void* p : own) std::free(p);
    return bad;
}

int main(int argc, char** argv)
{
    std::vector<Case> cases;
    for (int prec : {1, 2})
        for (int big = 0; big < 2; ++big) {   // argv group = 2 (prec - 1) + big
            const int C = big ? 128 : 64, R = big ? 4 : 2;
            const int F = ou_block_frames(C) - 2;
            if (!ou_block_up_supported(C, R, prec)) continue;
            // several windows with a ragged last one, exactly one window, shorter than the halo
            for (int T : {2 * F + 3 - (big ? 2 : 0), F, 3}) {
                cases.push_back({C, R, T, prec, false, false, 1, false, false, true});
                cases.push_back({C, R, T, prec, true, false, 2, true, true, true});
                cases.push_back({C, R, T, prec, true, true, 1, false, T != F, true});
            }
            cases.push_back({C, R, F + 5, prec, false, false, 0, false, true, false});   // plain transposed conv
        }
    const int only = argc > 1 ? std::atoi(argv[1]) : -1;
    int bad = 0, n = 0;
    for (const Case& c : cases) {
        if (only >= 0 && 2 * (c.prec - 1) + (c.C == 128) != only) continue;
        bad += run(c);
        ++n;
    }
    std::printf("%s: %d fused up-stage launches checked, %d bad\n", bad || !n ? "FAIL" : "ok", n, bad);
    return bad || !n ? 1 : 0;
}
