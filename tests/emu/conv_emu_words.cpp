// What ou_conv() answers to every tile word: one tiny geometry per kernel
// family, every word made of a shape id in 0..31 and any combination of bits
// 8-17, then -1.  Prints one character per word ('0' accepted, '1' / '2' the
// refusals -1 / -2, '?' anything else); accepted words run the emulated
// kernel under AddressSanitizer.  tests/test_conv_tile_words.py compares the
// line with the one recorded from the source before the host-side decoder
// (tests/golden/conv_tile_words.npz).
#ifdef OU_EMU_CONV_SRC   // another copy of the kernel source (tests/golden/make_conv_tile_words.py)
#include OU_EMU_CONV_SRC
#else
#include "../../open_universe_amd/csrc/ou_conv.hip"
#endif

#include <string>

struct Bufs {
    std::vector<float> wl, packed, x, y, bias, taps, ksws;
    std::vector<uint16_t> img;
};

// 0 f32, 1 split-f16, 2 split-f16 with a K-slice workspace, 3 split-f16 transposed (rout 2),
// 4 split-image input, 5 / 6 / 7 fir 1 (down, rate 2) / 2 (up, rate 2) / 3 (st_conv, stride 4)
static ou_conv_desc make(int c, Bufs& b)
{
    const int U = 64, fir = c >= 5 ? c - 4 : 0;
    const int cin = (fir == 1 || fir == 3) ? 16 : 32, cout = c == 0 || c == 4 ? 64 : 32;
    const int frame = fir == 1 ? 2 : fir == 3 ? 4 : 1, kt = fir ? 1 : 3;
    const int rout = c == 3 ? 2 : fir == 2 ? -2 : 1, phases = rout < 0 ? -rout : rout;
    const int T = U * frame, out_len = U * phases, m = cout * phases;
    const int mrows = fir == 2 ? (cout + 15) / 16 * 32 : m;   // fir 2: 32 / R whole channels per packed m-tile
    const int keff = cin * frame;
    b.wl.assign((size_t)mrows * keff * kt, 0.1f);
    b.packed.assign(ou_conv_packed_size(mrows, keff, kt, 0), 0.f);
    float unscale = 1.f;
    if (c == 0) ou_conv_pack(b.wl.data(), mrows, keff, kt, 0, b.packed.data());
    else if (c >= 4) ou_conv_pack_split_nat(b.wl.data(), mrows, keff, kt, b.packed.data(), &unscale);
    else ou_conv_pack_split(b.wl.data(), mrows, keff, kt, b.packed.data(), &unscale);
    b.x.assign((size_t)cin * T, 0.25f);
    b.y.assign((size_t)cout * out_len, 0.f);
    b.bias.assign(cout, 0.5f);
    ou_conv_desc d{};
    d.x = b.x.data(); d.x_bstride = (int64_t)cin * T; d.x_cstride = T;
    d.cin = cin; d.in_len = T; d.frame = frame; d.slope = 0.25f;
    d.w = b.packed.data(); d.m = m; d.kt = kt; d.pad = (kt - 1) / 2;
    d.n_frames = U; d.batch = 1; d.y = b.y.data(); d.y_bstride = (int64_t)cout * out_len; d.y_cstride = out_len;
    d.rout = rout; d.out_len = out_len; d.valid_len = out_len; d.bias = b.bias.data(); d.s1 = d.s2 = 1.f;
    d.prec = c == 0 ? 0 : 1; d.w_unscale = unscale; d.xs_shift = 6;
    if (c == 2) {
        b.ksws.assign(1 << 20, 0.f);
        d.ks_ws = b.ksws.data(); d.ks_ws_bytes = (int64_t)b.ksws.size() * 4;
    }
    if (c == 4) {
        const int rows = T + 3;
        b.img.assign((size_t)(cin / 32) * rows * 64, 0x3400);   // 0.25 in every half
        d.xs = b.img.data(); d.xs_bstride = (int64_t)(cin / 32) * rows * 128; d.xs_rows = rows;
    }
    if (fir) {
        b.taps.assign(2 * 2 + 1, 0.2f);
        d.fir = fir; d.fir_taps = fir == 3 ? nullptr : b.taps.data();
    }
    return d;
}

int main(int argc, char** argv)
{
    const int c = argc > 1 ? std::atoi(argv[1]) : 0;
    Bufs b;
    ou_conv_desc d = make(c, b);
    std::string codes;
    int accepted = 0;
    for (int i = 0; i <= 32768; ++i) {
        d.tile = i < 32768 ? (i & 31) | ((i >> 5) << OU_TILE_TPW_SHIFT) : -1;   // bits 8-17 from i >> 5
        const int rc = ou_conv(&d, nullptr);
        accepted += rc == 0;
        codes += rc == 0 ? '0' : rc == -1 ? '1' : rc == -2 ? '2' : '?';
    }
    std::printf("%s\n", codes.c_str());
    std::fprintf(stderr, "case %d: %d words accepted\n", c, accepted);
    return 0;
}
