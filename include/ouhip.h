/*
 * ouhip.h -- C ABI of the MI355X (gfx950) kernels behind open_universe_amd's
 * drop-in ``load_model()`` / ``model.enhance()`` surface.
 *
 * The reference (kolyangg/open-universe) is pure Python: its hot path is a
 * sequence of ATen ops issued from ``Universe.enhance``
 * (open_universe/networks/universe/universe.py:231-375) through the score and
 * conditioner networks.  Each entry point below replaces a run of those ops;
 * the reference interface it replaces is cited on each declaration.  The
 * Python host (open_universe_amd/_lib.py) binds these with ctypes.
 *
 * Conventions
 *  - All tensors are fp32 device pointers (caller-owned, hipMalloc'd or from
 *    the torch caching allocator); sizes are element counts; activations are
 *    NCW with the frame axis innermost (the reference's layout).
 *  - ``stream`` is a hipStream_t passed as void* (0 = null stream).
 *  - Every function returns 0 on success, a negative code on failure;
 *    ou_last_error() returns a thread-local message.  Nothing allocates device
 *    memory or synchronises, so every launch is hipGraph-capturable.
 */
#ifndef OUHIP_H
#define OUHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OUHIP_ABI_VERSION 11

int ou_abi_version(void);
const char* ou_last_error(void);

/* ------------------------------------------------------------------------
 * Fused implicit-GEMM 1-D convolution (kernels K1, K2, K3, K5, K8 of
 * SURVEY.md section 2.3).  Replaces PReLU_Conv.forward
 * (networks/universe/blocks.py:203-231) plus the ConvBlock arithmetic that
 * follows it (blocks.py:353-416: (h+res)/sqrt2, (cond_out+input_cond)/sqrt2,
 * film, conv stacks), the strided / transposed rate-change convolutions with
 * their binomial anti-alias FIRs folded into the weights (blocks.py:123-134,
 * 268-287), the 1x1 signal_cond_proj (score.py:166-171), the st_convs
 * (condition.py:33-65), the GRU input projection and the STFT-as-GEMM of the
 * mel front end (condition.py:85-108).
 *
 *   xv[c'][t] = prelu(in_scale[b] * x[b][c'%cin][t*R + c'/cin + shift])  (0 outside [0,in_len))
 *   (phase-major frame view: channel c' = ph*cin + ci; W's channel axis, as
 *   packed by ou_conv_pack, follows the same order)
 *   acc[m][u] = sum_{c',k} W[m][c'][k] * xv[c'][u + k - pad]     u in [f0, f0 + n_frames)
 *   m = ph*cout + co, t = u*rout + ph  (pixel shuffle; rout = 1 for plain convs)
 *   v = acc + bias[co];  v = t < valid_len ? v : 0
 *   v = (v + res1[b][co][t]) * s1;  v = film_g[b][co]*v + film_b[b][co];
 *   v = (v + res2[b][co][t]) * s2;  y[b][co][t] = v   for t < out_len
 * ---------------------------------------------------------------------- */

/* ou_conv_desc.tile: -1 = ou_conv's static choice (ou_conv_pick_tile), else
 * one word that selects the kernel family, its shape and its variants.  The
 * first of OU_TILE_FIR / _SS / _RS that is set names the family; without
 * them OU_TILE_WS, then a tiles-per-workgroup field > 0, then neither.
 *
 *   family             shape id (bits 0-7)  bits 8-9          other legal fields
 *   plain (one tile)   < ou_conv_num_tiles  0                 K slices, m-major
 *   persistent         same, no split-K     log2(tiles / WG)  -
 *   warp-specialised   same, ids 0-12       0                 -
 *   register-streamed  0-5                  diagnostic mode   K slices, m-major
 *   split-image        0-5 (NR - 1, + 3)    0                 m-major
 *   FIR                0-7                  early / deep      m-major
 *
 * Persistent and warp-specialised are f32 (prec 0) kernels and need f0 = 0;
 * register-streamed, split-image and FIR need prec 1 / 2 (split-image: 1).
 * K slices S > 1 need the workspace ks_ws.  ou_conv_tile_ok() says whether a
 * word is well formed and fits LDS at a tap count; ou_conv() itself also
 * takes the diagnostic modes, which ou_conv_tile_ok() refuses. */
#define OU_TILE_SHAPE_MASK 0xff
#define OU_TILE_TPW_SHIFT 8             /* plain: log2(output tiles per workgroup) */
#define OU_TILE_TPW_MASK (3 << 8)
#define OU_TILE_WS (1 << 10)            /* warp-specialised persistent kernel */
#define OU_TILE_SPLIT_QUERY (1 << 11)   /* ou_conv_tile_ok / ou_conv_lds_info only: */
                                        /* the plain shape's prec 1 / 2 form        */
#define OU_TILE_KS_SHIFT 12             /* log2(K slices S) */
#define OU_TILE_KS_MASK (3 << 12)
#define OU_TILE_RS (1 << 14)            /* register-streamed kernel */
#define OU_TILE_SS (1 << 15)            /* split-image input kernel (desc.xs) */
#define OU_TILE_MMAJOR (1 << 16)        /* m-groups fastest in the workgroup order */
#define OU_TILE_FIR (1 << 17)           /* FIR-applied rate-change kernels (desc.fir) */
#define OU_TILE_FIR_EARLY (1 << 8)      /* FIR, up (fir 2): epilogue loads before the main loop */
#define OU_TILE_FIR_DEEP (1 << 9)       /* FIR, lean down (fir 1) or up without EARLY: */
                                        /* two input chunks in flight per thread       */
#define OU_TILE_RS_DIAG_SHIFT 8         /* register-streamed: 1 no input loads, 2 no K loop */
#define OU_TILE_RS_DIAG_MASK (3 << 8)

typedef struct ou_conv_desc {
    const float* x;            /* input signal                                   */
    int64_t x_bstride;         /* elements between batch items                   */
    int64_t x_cstride;         /* elements between channels                      */
    int32_t cin;               /* underlying input channels                      */
    int32_t in_len;            /* valid samples per channel                      */
    int32_t frame;             /* R: frame-view factor (1 = plain NCW)           */
    int32_t shift;             /* sample offset of frame 0                       */
    const float* in_scale;     /* [B] per-item input multiplier, or NULL         */
    float slope;               /* scalar PReLU slope (1.0 = identity)            */
    const float* w;            /* weights packed by ou_conv_pack()               */
    int32_t m;                 /* GEMM rows = rout * cout                        */
    int32_t kt;                /* taps along frames: 1, 3, 4 or 5                */
    int32_t pad;               /* left padding in frames                         */
    int32_t cc;                /* channel chunk the weights were packed with     */
    int32_t n_frames;          /* output frames u                                */
    int32_t batch;
    float* y;
    int64_t y_bstride, y_cstride;
    int32_t rout;              /* output phases (transposed conv), 1 otherwise;  */
                               /* < 0: |rout| phases with channel-major rows     */
                               /* m = co * |rout| + ph (else m = ph * cout + co) */
    int32_t out_len;           /* store t < out_len                              */
    int32_t valid_len;         /* t >= valid_len stored as 0 before res1         */
    const float* bias;         /* [cout] or NULL                                 */
    const float* res1;         /* residual 1 or NULL                             */
    int64_t r1_bstride, r1_cstride;
    float s1;
    const float* film;         /* [B][2*cout] (gamma | beta) or NULL             */
    int64_t film_bstride;
    const float* res2;         /* residual 2 or NULL                             */
    int64_t r2_bstride, r2_cstride;
    float s2;
    int32_t tile;              /* -1 = auto, else an OU_TILE_* word (above)      */
    int32_t prec;              /* 0: f32 operands (weights from ou_conv_pack);   */
                               /* 1: split-f16 operands (ou_conv_pack_split),    */
                               /*    f32-class accuracy, see ou_conv.hip;        */
                               /* 2: f16 operands (the hi halves of the same     */
                               /*    packing), f32 accumulation                  */
    float w_unscale;           /* prec 1: power of two from ou_conv_pack_split   */
    int32_t f0;                /* first output frame u computed: the launch      */
                               /* covers u in [f0, f0 + n_frames), in the global */
                               /* frame coordinates of x / y (zero padding only  */
                               /* at the true ends); 0 = from the start.  The    */
                               /* persistent / warp-specialised f32 kernels      */
                               /* need f0 = 0                                    */
    int32_t* status;           /* prec 1 / 2: range codes (xs_shift) are OR-ed   */
                               /* in here, or NULL                               */
    float* ks_ws;              /* K-slice workspace (OU_TILE_KS_*: S > 1 slices) */
    int64_t ks_ws_bytes;       /* S partial sums per output tile, then           */
                               /* a reduce + epilogue launch; NULL if unused     */
    /* Split images (prec 1).  The operand of the NEXT conv, stored once by
     * its producer's epilogue so that the consumer stages it with plain
     * copies: for every stored y[b][co][t] (rout 1)
     *   p = prelu_{sy_slope}(y) * 2^-sy_shift,  hi = f16(p),
     *   lo = f16((p - hi) * 2^11)
     * at byte (co / 32 * sy_rows + t) * 128 + (co % 32) * 2 (hi) and + 64
     * (lo) of item b: one 128-B row per 32-channel block and sample, the
     * channels of a block consecutive.  |p| >= 2^15 sets *status. */
    uint16_t* sy;              /* producer: also store y's split image, or NULL  */
                               /* (rout 1, m % 32 == 0, prec 1)                  */
    int64_t sy_bstride;        /* bytes between batch items                      */
    int32_t sy_rows;           /* samples per 32-channel block (>= out_len)      */
    int32_t sy_shift;          /* the consumer's staging exponent                */
    float sy_slope;            /* the consumer's PReLU slope                     */
    int32_t sy_pad_;
    const uint16_t* xs;        /* consumer (OU_TILE_SS, conv_skernel): read the  */
                               /* PReLU'd operand from this split image instead  */
                               /* of x (x, slope and in_scale unused; weights    */
                               /* from ou_conv_pack_split_nat; cin % 32 == 0)    */
    int64_t xs_bstride;        /* bytes between batch items                      */
    int32_t xs_rows;           /* samples per 32-channel block (>= in_len)       */
    int32_t xs_shift;          /* staging exponent s of every split-f16 / f16    */
                               /* kernel: the operand is staged (with xs: was    */
                               /* stored) as prelu(x) * 2^-s, |.| < 2^15.  A     */
                               /* larger staged value sets range code 1 in       */
                               /* *status, a larger split-image value (sy) 2, an */
                               /* infinite one 4; the engine then widens that    */
                               /* layer's exponent (default 6).  Bits 8 / 9 / 10 */
                               /* (with 1 / 2, ou_block's codes too): a finite   */
                               /* staged value reached 2^23 / 2^31 / 2^39        */
    /* Anti-aliased rate-change convs with the binomial FIR applied instead of
     * folded into the weights (OU_TILE_FIR; PReLU_Conv with use_antialiasing,
     * blocks.py:214-226, BinomialAntiAlias blocks.py:123-134):
     *   fir 1: f = FIR(prelu(x)) ('same', zero outside [0, in_len)), then the
     *          strided conv over f's frame view: frame = R, rout 1, K = cin R;
     *   fir 2: the transposed conv (frame 1, rout = -R, K = cin), then the FIR
     *          over its R * in_len output samples (zero outside), then bias.
     *   fir 3: no FIR: a plain strided conv (frame = R any multiple of 4,
     *          rout 1, K = cin R; the st_convs, condition.py:53-59) in fir 1's
     *          K order, walked so that each input sample is read once;
     * R is 2, 3, 4, 5 or 8 (fir 1 / 2); kt 1, pad 0, shift 0, no in_scale, no
     * xs; prec 1 or 2; weights w_logical[m'][k] packed by
     * ou_conv_pack_split_nat(kt 1):
     *   fir 1, 3: m' = co (m = cout rows), K in chunks of 16 channels x Q
     *          phases (Q = R for fir 1; 8 if R % 8 == 0 else 4 for fir 3),
     *          channel-major inside a chunk:
     *          k = ((cb R / Q + s) 16 + c) Q + p  for input channel
     *          ci = 16 cb + c (cin % 16 == 0) and conv tap ph = s Q + p
     *          (fir 1: k = ci R + ph, the frame view's order);
     *   fir 2: every 32-row m-tile holds P = 32 / R whole channels, row
     *          m' = 32 (co / P) + (co % P) R + ph (rows past P R zero), so
     *          ceil(cout / P) * 32 packed rows; k = ci (cin % 32 == 0).
     * fir 0: the other kernels (FIR folded into the weights). */
    int32_t fir;
    int32_t fir_pad_;
    const float* fir_taps;     /* [2R + 1] FIR taps (device; fir 1 / 2)          */
} ou_conv_desc;

/* Default channel chunk of the kernel for a tap count (informational: the
 * packed weight layout does not depend on it). */
int ou_conv_chunk(int kt, int frame);
/* Number of floats of the packed weight buffer. */
int64_t ou_conv_packed_size(int m, int cin_eff, int kt, int cc);
/* Host-side packing: w_logical[m][cin_eff][kt] (row-major, host memory)
 * -> packed[] in the per-lane MFMA fragment order the kernel streams:
 * [m-tile of 32][pair / 4][tap][lane][pair % 4], lane l holding row l & 31
 * and channel 2*pair + (l >> 5); channels padded with zeros to a multiple of
 * 64 (one float4 per lane = 4 consecutive k-steps of the MFMA stream). */
int ou_conv_pack(const float* w_logical, int m, int cin_eff, int kt, int cc,
                 float* packed);
/* Split-f16 packing (prec 1): the same number of floats as ou_conv_pack, in
 * the order [m-tile][8-pair group][hi | lo][tap][lane][8 halves] (lane l:
 * row l & 31, channel 2*(8*group + j) + (l >> 5) in half j) of
 * a = w * 2^e, hi = f16(a), lo = f16((a - hi) * 2^11), with e chosen per
 * layer so max|a| lies in [2^9, 2^10).  *w_unscale receives 2^(6-e) (the
 * kernel stages the input as x * 2^-6). */
int ou_conv_pack_split(const float* w_logical, int m, int cin_eff, int kt,
                       float* packed, float* w_unscale);
/* The same, in the natural channel order of the split-image kernel
 * (OU_TILE_SS): [m-tile][16-channel group g][hi | lo][tap][lane][8 halves], lane l
 * holding row l & 31 and channel 16*g + 8*(l >> 5) + j in half j -- a lane's
 * B operand is then 8 consecutive channels of one split-image row. */
int ou_conv_pack_split_nat(const float* w_logical, int m, int cin_eff, int kt,
                           float* packed, float* w_unscale);
int ou_conv(const ou_conv_desc* d, void* stream);
/* The tile configuration ou_conv would use for this descriptor when
 * d->tile < 0; ou_conv_num_tiles() configurations exist, ou_conv_tile_ok()
 * says whether one fits the LDS budget for a tap count (host autotuning
 * times the valid ones per layer and stores the winner in d->tile). */
int ou_conv_pick_tile(const ou_conv_desc* d);
int ou_conv_num_tiles(void);
int ou_conv_tile_ok(int kt, int tile);
/* Diagnostics: LDS bytes a tile shape requests at tap count kt, and the
 * device's opt-in per-workgroup LDS limit. */
int ou_conv_lds_info(int kt, int tile, int* lds_request, int* device_optin_max);

/* ------------------------------------------------------------------------
 * Bidirectional GRU recurrence (kernel K6).  Replaces the recurrent part of
 * torch.nn.GRU in ScoreEncoder (score.py:84-90,117-118) and
 * ConditionerEncoder (condition.py:173-179,212-215).  The input projection
 * gi = W_ih x + b_ih is produced beforehand by ou_conv (1x1) into
 * gi[b][dir*3H + gate*H + j][t].  One persistent launch per layer: H/32
 * workgroups per direction hold W_hh in registers and hand h_t between
 * workgroups through 8-byte {tag, value} granules (bounded spins).
 *   y[b][dir*H + j][t] = (h + res[b][dir*H + j][t]) * res_scale   (res optional)
 * ---------------------------------------------------------------------- */
typedef struct ou_gru_desc {
    const float* gi;           /* [B][2*3H][T]                                    */
    int64_t gi_bstride;
    const float* w_hh;         /* [2][3H][H] (direction-major, torch layout)      */
    const float* b_hh;         /* [2][3H]                                         */
    float* y;                  /* [B][2H][T] (strides below)                      */
    int64_t y_bstride, y_cstride;
    const float* res;          /* optional residual, same layout as y             */
    int64_t res_bstride, res_cstride;
    float res_scale;
    int32_t hidden;            /* H: 256 or 384                                   */
    int32_t steps;             /* T                                               */
    int32_t batch;
    int32_t flags;             /* -1 default; bit0 XCD-local chains, bit1 spin    */
                               /* without s_sleep, bit2 64-unit workgroups, bit3  */
                               /* 128-unit workgroups, bit4 timing diagnostic     */
                               /* (skips the hand-off wait: wrong results), bit5  */
                               /* the workgroup-gather kernel instead of the      */
                               /* k-split one (whole sequences only), bit6 no     */
                               /* placement handshake (k-split kernel: every      */
                               /* hand-off store is write-through; ou_gru sets it */
                               /* itself for a launch of one step), bit7 8 units  */
                               /* per wave instead of 4 (k-split kernel), bit8    */
                               /* per-step gi prefetch instead of LDS-staged gi   */
                               /* chunks (one item per chain), bit9 the earlier   */
                               /* step loop of the k-split kernel instead of the  */
                               /* straight-line one (one item per chain: packed   */
                               /* dot products, peeled first / last step, no      */
                               /* run-time branches; same bits in y and hstate;   */
                               /* bits 1 and 8 imply bit9); bits 12-14 XCD offset */
                               /* of the bit-0 chain layout, bit 15 keeps the     */
                               /* defaults of bits 0-11                           */
    uint64_t* granules;        /* workspace: ou_gru_workspace_bytes()             */
    int32_t* status;           /* device int, set nonzero on spin timeout         */
    int32_t t_begin, t_end;    /* steps [t_begin, t_end) of the T-step sequences  */
                               /* (forward: time t, backward: T - 1 - t); 0, 0 =  */
                               /* all.  A launch with t_begin > 0 starts from     */
                               /* hstate; every launch leaves h of its last step  */
                               /* there: the recurrence split over launches, each */
                               /* ordered after the one before (k-split kernel).  */
                               /* A continuing range (t_begin > 0) holds at least */
                               /* two steps: one step is refused (-2), because    */
                               /* only a step's hand-off orders the workgroups'   */
                               /* hstate stores after each other's loads.  One    */
                               /* step from t_begin == 0 (T == 1 included) runs   */
                               /* without the placement handshake (flags bit6)    */
    float* hstate;             /* [B][2][H], or NULL (whole sequences only)       */
    int32_t ws_zeroed;         /* nonzero: the caller zeroed the workspace before */
                               /* the first launch on it (per replay); launches   */
                               /* leave it reusable, so no per-launch memset --   */
                               /* launches of steps < 5 clear it before and after */
                               /* they run (the tags T-1, T-2 a launch leaves     */
                               /* must not match a new launch's first two polls,  */
                               /* tags 1 and 2): launches of any T may share it   */
    int32_t _pad;
} ou_gru_desc;

int64_t ou_gru_workspace_bytes(int hidden, int batch);
/* k-split kernel: the workgroups one launch keeps resident.  A batch whose
 * chains (2 per item, hidden / 16 or hidden / 32 workgroups each) exceed it
 * runs several items per chain, then several launches. */
int ou_gru_ks_max_workgroups(void);
int ou_gru(const ou_gru_desc* d, void* stream);

/* ------------------------------------------------------------------------
 * Noise-level embedding + every FiLM projection of the score network for a
 * list of sigma values (kernel K7).  Replaces SimpleTimeEmbedding /
 * SigmaBlock (sigma_block.py:24-78) and the per-level
 * Linear(noise_cond_dim -> 2C) calls (score.py:104-110,197-210).
 *   g = embed(log10(sigma[i]));  out[i][r] = sum_k W[r][k] g[k] + bias[r]
 * ---------------------------------------------------------------------- */
typedef struct ou_embed_desc {
    const float* sigma;        /* [n] noise levels (already scaled by edm.noise) */
    int32_t n;
    int32_t kind;              /* 0 = SimpleTimeEmbedding, 1 = SigmaBlock RFF    */
    int32_t dim;               /* noise_cond_dim (512)                           */
    float te_weight, te_bias;  /* SimpleTimeEmbedding scalars                    */
    const float* rff_freq;     /* SigmaBlock: [n_rff]                            */
    int32_t n_rff;
    int32_t rows;              /* total projection rows                          */
    const float* mlp_w[3];     /* SigmaBlock Linear weights (out x in)           */
    const float* mlp_b[3];
    float mlp_slope[3];
    const float* w;            /* [rows][dim] concatenated projections           */
    const float* bias;         /* [rows]                                         */
    float* out;                /* [n][rows]                                      */
    float* gbuf;               /* scratch [n][dim]                               */
} ou_embed_desc;

int ou_embed(const ou_embed_desc* d, void* stream);

/* ------------------------------------------------------------------------
 * Score-network head fused with the EDM wrapper and the sampler update
 * (kernel K9).  Replaces ScoreNetwork.forward's last two lines
 * (score.py:290-296: prelu -> output_conv), Universe._edm_score_wrapper
 * (universe.py:197-209) and the update lines of the diffusion loop
 * (universe.py:334-343).
 *   net = conv3(prelu2(prelu1(h)))[b][t] + bias
 *   mode 0: out = net
 *   else:   score = edm ? ((w_skip*x + w_out*net) - x) / s2 : net
 *   mode 1: out = (x + c_score*score) + c_noise*(z*s_next)
 *   mode 2: out = x + c_score*score
 * ---------------------------------------------------------------------- */
typedef struct ou_head_desc {
    const float* h;            /* [B][C][T] decoder output                       */
    int64_t h_bstride;
    int32_t channels, length, batch, mode;
    float slope1, slope2;
    const float* w;            /* [C][3] folded output_conv weight               */
    float bias;
    int32_t edm, _pad;
    float w_skip, w_out, s2, c_score, c_noise, s_next;
    const float* x;            /* [B][T] current sample (may alias out)          */
    const float* z;            /* [B][T] standard normal noise or NULL           */
    float* out;                /* [B][T]                                         */
} ou_head_desc;

int ou_head(const ou_head_desc* d, void* stream);

/* ------------------------------------------------------------------------
 * Row statistics and elementwise helpers around the sampler
 * (kernel K9): normalize_batch (utils/norm.py:47-87), the mel
 * normalization (condition.py:104-106), pad / unpad / peak-normalize /
 * keep_rms (universe.py:259,267-270,349-357).
 * ---------------------------------------------------------------------- */
/* y[b][i] = (x[b][i] - mean_b) * (level / max(std_b, eps)); std unbiased. */
int ou_normalize(const float* x, float* y, int batch, int64_t n, float level,
                 float eps, void* stream);
/* out[b] = 1 / max(sqrt(sum_i x[b][i]^2 / denom), eps)  (mel normalisation) */
int ou_inv_rms(const float* x, float* out, int batch, int64_t n, float denom,
               float eps, void* stream);
/* out[b] = sqrt(mean_i x[b][i]^2)                                          */
int ou_rms(const float* x, float* out, int batch, int64_t n, void* stream);
/* y[b][f][t] = x[b][f][t]^2 + x[b][f+F][t]^2   (|STFT|^2 from re/im rows)   */
int ou_power(const float* x, float* y, int batch, int nf, int frames, void* stream);
/* y[b][t] = x[b][t - left] for t-left in [0, n_in), 0 otherwise; len n_out  */
int ou_pad(const float* x, int64_t x_bstride, float* y, int batch, int n_in,
           int n_out, int left, void* stream);
/* y[i] = z[i] * scale (+ add[i])  (initial sample x0 = randn * sigma_0, or
 * the warm start aux + randn * sigma_k, universe.py:322-331)              */
int ou_scale(const float* z, float* y, int64_t n, float scale, const float* add,
             void* stream);
/* enhance() tail: crop [left, left+len) of x (stride x_bstride), optional
 * keep_rms rescale (mix_rms[b] / max(rms(x_b), 1e-5)), then divide by the
 * peak when it exceeds 1.                                                 */
int ou_finish(const float* x, int64_t x_bstride, int left, float* y, int batch,
              int len, const float* mix_rms, void* stream);
/* Elementwise median / mean over an ensemble of E results, [E][n] -> [n]
 * (universe.py:359-366: x.mean(dim=0) / x.median(dim=0).values, lower median). */
int ou_ensemble_reduce(const float* x, float* y, int ensemble, int64_t n,
                       int mode /* 0 mean, 1 median */, void* stream);
/* Ensemble signal_median (universe.py:366-367 -> utils/stats.py:22-66):
 * x [E][batch][n] -> y [batch][n] = the member selected by the reference's
 * per-sample rank vote.  counts: device int32 workspace [batch][32] (zeroed
 * here).  E <= 32. */
int ou_signal_median(const float* x, float* y, int ensemble, int batch, int64_t n, int* counts,
                     void* stream);

/* Audio-rate resampling around enhance(): replaces
 * torchaudio.functional.resample(x, orig, new) with its defaults
 * (sinc_interp_hann, lowpass width 6, rolloff 0.99) that the reference CLI
 * applies before and after the model (bin/enhance.py:61-64, 186-190).
 * orig/new reduced by their gcd; kernel = [phases = new][taps = 2*width + orig]
 * (dsp.sinc_resample_kernel); n_out = ceil(new * n_in / orig). */
int ou_resample(const float* x, int64_t x_bstride, float* y, int64_t y_bstride, int batch, int n_in,
                int n_out, const float* kernel, int phases, int taps, int orig, int width, void* stream);

/* FLAC input decoding for the CLI (host code): the
 * reference reads .wav/.mp3/.flac with torchaudio.load (bin/enhance.py:33,
 * 61-64); libFLAC / torchaudio are absent here.  ou_flac_info parses
 * STREAMINFO (frames = total samples per channel; counted by a decode pass
 * when STREAMINFO leaves it 0).  ou_flac_decode writes planar float32
 * out[c * frames + i] = sample / 2^(bps-1) (torchaudio.load's scaling) and
 * returns the frames decoded, or < 0 (ou_last_error) on a malformed stream or
 * a CRC-8 / CRC-16 mismatch. */
int ou_flac_info(const uint8_t* data, int64_t n, int32_t* sample_rate, int32_t* channels,
                 int32_t* bits_per_sample, int64_t* frames);
int64_t ou_flac_decode(const uint8_t* data, int64_t n, float* out, int64_t frames);
/* FLAC output (a .flac input is written back as .flac, as torchaudio.save
 * does): x planar float32 [channels][frames], PCM of bps = 16 or 24 bits
 * (round(x * 2^(bps-1)), clamped), FIXED-2 / VERBATIM subframes, CRCs set.
 * Returns the bytes written (<= ou_flac_encode_bound) or < 0. */
int64_t ou_flac_encode_bound(int channels, int64_t frames, int bps);
int64_t ou_flac_encode(const float* x, int channels, int64_t frames, int sample_rate, int bps, uint8_t* out,
                       int64_t capacity);

/* Alias-free Snake of the signal-decoupling layer (universe_gan.py:119-151;
 * bigvgan/snake.py:131-157, alias_free_act.py:8-30): torchaudio-style 2x
 * sinc up-sampling, Snake x + sin^2(a x)/(a + 1e-9), 2x down-sampling.  The
 * Conv1d(C -> 1, k3) that follows is ou_head in mode 0 with unit slopes.
 *   u[2s+i] = sum_k k_up[i][k] h[s+k-width_up];  y[t] = sum_k k_down[k] v[2t+k-width_down] */
typedef struct ou_snake_desc {
    const float* h;            /* [B][C][T]                                      */
    int64_t h_bstride;
    int32_t channels, length, batch, _pad0;
    const float* alpha;        /* [C] exp(log_alpha)                             */
    const float* k_up;         /* [2][taps_up]                                   */
    int32_t taps_up, width_up;
    const float* k_down;       /* [taps_down]                                    */
    int32_t taps_down, width_down;
    float* out;                /* [B][C][T]                                      */
} ou_snake_desc;

int ou_snake_aa(const ou_snake_desc* d, void* stream);

/* ------------------------------------------------------------------------
 * Fused ConvBlock main path (ou_block.hip): the three PReLU_Conv calls of a
 * ConvBlock and the arithmetic between them in one launch, for channel
 * counts whose whole channel range fits one workgroup (32, 64, 128, and
 * PP24's 48, 96 and 192; 256 and
 * 512 stay on ou_conv, see ou_block_supported) and
 * split-f16 / f16 / f32 operands.  Replaces blocks.py:393-416:
 *   c1 = conv1(h) (k5);  c1 = (c1 + sc) * s_sc;  c1 = film(c1);  cond_out = c1
 *   y  = ((h + conv3(conv2(c1))) * s_res + res2) * s2        (k3, k3)
 * Each conv applies its scalar PReLU slope to its input; frames outside
 * [0, length) are zero padding.  sc / film / cond_out / res2 are optional
 * (NULL).  y must not alias h, sc, cond_out or res2.
 * Optional fourth stages on the block output, inside the same launch: the
 * score head (head), the encoder's strided rate-change conv (w_down) and
 * the decoder's up-sampling conv of the next level (w_up: y -> u, with the
 * skip residual added in place and y itself not stored when NULL).
 * ---------------------------------------------------------------------- */
typedef struct ou_block_desc {
    const float* h;            /* block input [B][C][T]                          */
    int64_t h_bstride, h_cstride;
    int32_t channels, length;  /* C, T                                           */
    int32_t batch, prec;       /* prec 0 f32, 1 split-f16, 2 f16                 */
    const void* w[3];          /* conv1 (k5), conv2, conv3 (k3): ou_block_pack   */
    const float* bias[3];      /* [C] or NULL                                    */
    float slope[3];            /* PReLU slope on each conv's input               */
    float w_unscale[3];        /* from ou_block_pack                             */
    const float* sc;           /* conv1 residual (input_cond) or NULL            */
    int64_t sc_bstride, sc_cstride;
    float s_sc;
    int32_t dbg;               /* diagnostics only (tools/block_bench.py): 0     */
    const float* film;         /* [B][2C] (gamma | beta) or NULL                 */
    int64_t film_bstride;
    float* cond_out;           /* conv1 result after sc / FiLM, or NULL          */
    int64_t co_bstride, co_cstride;
    float* y;
    int64_t y_bstride, y_cstride;
    float s_res, s2;
    const float* res2;         /* or NULL                                        */
    int64_t r2_bstride, r2_cstride;
    int32_t* status;           /* split-f16 range flag (as ou_conv), or NULL     */
    /* 32 and 48 channels (the score network's level-0 blocks of PP16 / PP24;
     * with w_down as well, 32 only), the score network's ends (both optional,
     * NULL = off):
     * the block input is h = conv1d(in_scale[b] * x, w_in, b_in) (score
     * input_conv, 1 -> C, k3, score.py:244-246,285) instead of reading h;
     * and/or the block output goes through the score head (ou_head fields of
     * `head`; head.h is ignored) instead of being stored to y.            */
    const float* x;            /* [B][T] sampler state                           */
    int64_t x_bstride;
    const float* in_scale;     /* [B] or NULL                                    */
    const float* w_in;         /* [C][3]                                         */
    const float* b_in;         /* [C]                                            */
    ou_head_desc head;         /* head.w == NULL: no head                        */
    /* 32 / 64 channels (ou_block_down_supported): the encoder's strided
     * rate-change conv (blocks.py:203-231,268-275) on the block output, which
     * is still stored to y: e = conv(PReLU_down(y)) with stride `rate` and 2C
     * output rows over down_kt frames of `rate` samples per output frame
     * (down_kt 3: the anti-alias FIR folded in, frames -1, 0, +1; down_kt 1:
     * plain), zero outside [0, length).                                     */
    const void* w_down;        /* ou_block_pack_rect(2C, C, down_kt * rate) of
                                  the tap-major weights (tap k * rate + phase),
                                  or NULL: no rate-change conv                   */
    const float* b_down;       /* [2C] or NULL                                   */
    float slope_down, w_down_unscale;
    int32_t rate, down_kt;
    float* e;                  /* [B][2C][ceil(length / rate)]                   */
    int64_t e_bstride, e_cstride;
    /* Frame range (a chunk of a longer signal): outputs (y, cond_out, the
     * head, e) are computed and stored for frames [f0, f1) only, reading h
     * (x) wherever the convs' halos reach -- zero padding stays at [0,
     * length).  f1 = 0: the whole signal.  With a rate-change conv f0 and f1
     * are multiples of `rate`.  h frames outside [h0, h1) are read as zero
     * (h1 = 0: no limit): a chunk's caller has produced h only there, and
     * the frames it leaves out reach no stored output -- a workgroup past f1
     * stages them but stores nothing they feed.                             */
    int32_t f0, f1;
    int32_t h0, h1;
    /* Staging exponents (prec 1 / 2) of the conv1, conv2, conv3 and rate-
     * change conv inputs: each is staged as prelu(v) * 2^-shift (|.| < 2^15;
     * a larger value sets range code 1 / 2 / 8 / 16 in *status, an infinite
     * one 4).  The engine uses 6 unless a range flag widened a stage. */
    int32_t shift[4];
    /* Split images (prec 1; layout and values as ou_conv_desc.sy / xs).  sy:
     * also store the block output's image for the next conv (y is stored
     * too; not with a head; range code 32 when a value leaves the range).
     * xs: stage 0 copies the conv1 operand from this image (stored by the
     * producing conv with slope[0] and shift[0]) instead of staging h, which
     * is then read only as the residual (whole signal: f0 = f1 = h0 = h1 = 0,
     * no input conv). */
    uint16_t* sy;
    int64_t sy_bstride;        /* bytes between batch items                      */
    int32_t sy_rows, sy_shift; /* samples per 32-channel block; exponent        */
    float sy_slope;            /* the consumer's PReLU slope                     */
    int32_t sy_pad_;
    const uint16_t* xs;
    int64_t xs_bstride;        /* bytes between batch items                      */
    int32_t xs_rows, xs_pad_;  /* samples per 32-channel block (>= length)       */
    /* 64 / 128 channels, prec 1 / 2 (ou_block_up_supported): the decoder's
     * up-sampling PReLU_Conv that consumes the block output (blocks.py:221-225,
     * 276-283) as a fourth stage, the FIR-applied form of ou_conv_desc.fir 2:
     *   z[t up_rate + ph][co] = sum_ci w[ci][co][ph] PReLU_up(y)[t][ci]
     *   v = FIR(z) (2 up_rate + 1 taps, 'same', z zero outside [0, up_rate *
     *       length)) + b_up;   v = 0 at samples >= u_valid
     *   u = (v + u_res) * s_u                      for samples < u_len
     * A workgroup then owns ou_block_frames(C) - 2 frames (one halo frame of y
     * on each side feeds the FIR).  up_taps NULL: no FIR (a plain transposed
     * conv).  u_res NULL: no residual (s_u still applies); u_res may alias u
     * exactly (the in-place skip add: each element is read and written by the
     * same thread).  u must not alias h, sc, y or res2.  With w_up set, y may
     * be NULL (the block output is not stored), the whole signal is computed
     * (f0 = f1 = h0 = h1 = 0) and sy, head and w_down are not combined.  The
     * PReLU_up(y) operand is staged with shift[3]; range code 16.           */
    const void* w_up;          /* ou_block_pack_rect(up_rate * C / 2, C, 1) of the
                                  rows 32 (co / P) + (co % P) up_rate + ph, P =
                                  32 / up_rate (the fir 2 row order of
                                  ou_conv_desc), or NULL: no up conv            */
    const float* b_up;         /* [C / 2] or NULL                                */
    const float* up_taps;      /* [2 up_rate + 1] or NULL                        */
    float slope_up, w_up_unscale;
    int32_t up_rate, up_pad_;
    float* u;                  /* [B][C / 2][>= u_len]                           */
    int64_t u_bstride, u_cstride;
    int32_t u_len, u_valid;    /* samples stored (<= up_rate * length); zero-fill
                                  from u_valid on                                */
    const float* u_res;        /* skip residual or NULL                          */
    int64_t ur_bstride, ur_cstride;
    float s_u;
    int32_t u_pad2_;
} ou_block_desc;

/* 1 when ou_block handles this channel count and operand precision. */
int ou_block_supported(int channels, int prec);
/* Output frames per workgroup (the grid is ceil(length / frames) x batch). */
int ou_block_frames(int channels);
/* Halves of one packed conv (C x C x kt, hi and lo planes). */
int64_t ou_block_packed_halves(int channels, int kt);
/* Pack w[C][C][kt] (f32, host) as [m-tile][tap][16-channel step][hi | lo]
 * [lane][8 halves] of a = w * 2^e (max|a| in [2^9, 2^10)); *w_unscale =
 * 2^(6 - e). */
int ou_block_pack(const float* w, int channels, int kt, void* out, float* w_unscale);
/* The same packing for w[m][channels][kt] (m % 32 == 0, channels % 16 == 0):
 * the fused rate-change conv's 2C x C x (down_kt * rate) weights.            */
int ou_block_pack_rect(const float* w, int m, int channels, int kt, void* out, float* w_unscale);
/* f32 operands (prec 0): floats of the packed conv, and the packing
 * [m-tile][tap][4 channel pairs][lane][4] (lane l: row l & 31, channel
 * 2 pair + (l >> 5); rows padded to 32); *w_unscale = 2^6. */
int64_t ou_block_packed_f32(int channels, int kt);
int ou_block_pack_f32(const float* w, int channels, int kt, float* out, float* w_unscale);
/* 1 when ou_block fuses the rate-change conv for (channels, rate, kt, prec). */
int ou_block_down_supported(int channels, int rate, int kt, int prec);
/* 1 when ou_block fuses the up-sampling conv for (channels, rate, prec). */
int ou_block_up_supported(int channels, int rate, int prec);
int ou_block(const ou_block_desc* d, void* stream);

/* ------------------------------------------------------------------------
 * Program: a recorded list of the launches above, replayed natively (and
 * optionally as one hipGraph).  Built once per (shape, options) by the
 * Python host; replaces the Python-level loop of Universe.enhance.
 * ---------------------------------------------------------------------- */
typedef struct ou_program ou_program;

enum {
    OU_OP_CONV = 1, OU_OP_GRU = 2, OU_OP_EMBED = 3, OU_OP_HEAD = 4,
    OU_OP_NORMALIZE = 5, OU_OP_INV_RMS = 6, OU_OP_POWER = 7, OU_OP_PAD = 8,
    OU_OP_SCALE = 9, OU_OP_FINISH = 10, OU_OP_RMS = 11, OU_OP_SNAKE = 12,
    OU_OP_MEMSET = 13, OU_OP_ENSEMBLE = 14, OU_OP_BLOCK = 15,
    /* lanes: ops after OU_OP_LANE{id} run on stream `id` (0 = the caller's /
     * capture stream, id > 0 = program-owned side streams); OU_OP_SIGNAL{id}
     * records event id on the current lane, OU_OP_WAIT{id} makes the current
     * lane wait for it.  A side lane must start with a WAIT and lane 0 must end
     * after waiting for every side lane's last SIGNAL (checked: run and
     * capture fail otherwise).  ou_program_profile runs the list serially. */
    OU_OP_LANE = 16, OU_OP_SIGNAL = 17, OU_OP_WAIT = 18
};

/* Descriptors of the helper ops when recorded into a program. */
typedef struct ou_memset_desc {
    void* ptr;
    int64_t bytes;
} ou_memset_desc;
typedef struct ou_norm_args {
    const float* x;
    float* y;
    int32_t batch, _pad;
    int64_t n;
    float level, eps;
} ou_norm_args;
typedef struct ou_rms_args {
    const float* x;
    float* out;
    int32_t batch, _pad;
    int64_t n;
    float denom, eps;
} ou_rms_args;
typedef struct ou_power_args {
    const float* x;
    float* y;
    int32_t batch, nf, frames, _pad;
} ou_power_args;
typedef struct ou_pad_args {
    const float* x;
    int64_t x_bstride;
    float* y;
    int32_t batch, n_in, n_out, left;
} ou_pad_args;
typedef struct ou_scale_args {
    const float* z;
    float* y;
    int64_t n;
    float scale, _pad;
    const float* add;
} ou_scale_args;
typedef struct ou_finish_args {
    const float* x;
    int64_t x_bstride;
    int32_t left, batch, len, _pad;
    float* y;
    const float* mix_rms;
} ou_finish_args;
typedef struct ou_sync_args {
    int32_t id;                /* lane 0..8 (OU_OP_LANE) or event 0..4095 */
    int32_t _pad;
} ou_sync_args;
typedef struct ou_ensemble_args {
    const float* x;
    float* y;
    int32_t ensemble, mode;    /* mode 0 mean, 1 median, 2 signal_median   */
    int64_t n;                 /* batch * samples                          */
    int32_t batch, _pad;       /* signal_median: batch items (n / batch each) */
    int32_t* counts;           /* signal_median: [batch][32] int32 workspace */
} ou_ensemble_args;

ou_program* ou_program_create(void);
void ou_program_destroy(ou_program* p);
/* op-specific descriptor, copied into the program. */
int ou_program_add(ou_program* p, int op, const void* desc, size_t desc_bytes);
/* Replace the descriptor of op `index` (same kind and size; drops a captured
 * graph).  The recorder uses it to give a conv's epilogue a split-image
 * output (ou_conv_desc.sy) once it sees the conv that consumes it. */
int ou_program_patch(ou_program* p, int index, int op, const void* desc, size_t desc_bytes);
int ou_program_size(const ou_program* p);
int ou_program_run(ou_program* p, void* stream);
/* Capture the program into a hipGraph (on a private stream) and instantiate. */
int ou_program_capture(ou_program* p);
/* Host-only check of the lane structure (what run / capture validate
 * first): 0, or < 0 with ou_last_error.  No HIP call.                      */
int ou_program_validate(const ou_program* p);
/* Capture every maximal run of kernels on one lane (between two sync ops)
 * as its own hipGraph instead; ou_program_launch then replays the lanes on
 * real streams with host-side events, one graph launch per run.            */
int ou_program_capture_segments(ou_program* p);
/* Launch the captured program (whole graph, or segments) on ``stream``. */
int ou_program_launch(ou_program* p, void* stream);
/* Kind (OU_OP_*) of op i. */
int ou_program_op_kind(const ou_program* p, int i);
/* Eager replay with a hipEvent pair around every op on ``stream``; writes the
 * per-op device time in milliseconds to ms[0..size) (synchronises).  Used by
 * bench.py to attribute time to kernels inside the same workload. */
int ou_program_profile(ou_program* p, void* stream, float* ms);
/* Eager replay with the lanes on their streams (as ou_program_run) and a
 * hipEvent before and after every op on its lane: t0[i] / t1[i] = ms from the
 * replay's start to when op i's lane reached / finished it, -1 for sync ops
 * (synchronises).  The concurrent timeline of the lane schedule
 * (tools/critical_path.py). */
int ou_program_trace(ou_program* p, void* stream, float* t0, float* t1);

/* ------------------------------------------------------------------------
 * Sampler noise: a counter-based normal stream of the project's own (it does
 * not reproduce torch.randn).  Philox4x32-10 with key = (seed low, seed high)
 * and counter = (q low, q high, 0, 0), q = offset + i / 4: counter q yields
 * out[4 (q - offset) .. + 4).  From the four words x0..x3,
 *   u1 = ((x0 >> 8) + 1) 2^-24,  u2 = (x1 >> 8) 2^-24      (exact in f32)
 *   r = sqrtf(-2 logf(u1)),  z0 = r cospif(2 u2),  z1 = r sinpif(2 u2)
 * and (x2, x3) give (z2, z3) the same way.  ou_randn launches one kernel on
 * ``stream``; ou_philox4x32 is the generator's block function on the host
 * (10 rounds, Random123's known answers).
 * ---------------------------------------------------------------------- */
int ou_randn(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream);
int ou_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);

/* ------------------------------------------------------------------------
 * Exported enhance bundles: one recorded enhance program for a fixed
 * (batch, length, options) in a relocatable file (written by
 * open_universe_amd/bundle.py), replayed without Python.
 *
 * File layout (little-endian; every section starts on a 64-byte boundary):
 *   header, 128 bytes
 *       0 char[4] "OUHB"    4 u32 format version (1)   8 u32 OUHIP_ABI_VERSION
 *      12 u32 regions      16 u32 ops                 20 u32 relocations
 *      24 u32 JSON bytes   28 u32 0                   32 char[16] arch ("gfx950")
 *      48 u64 region table 56 u64 op table            64 u64 relocation table
 *      72 u64 I/O table    80 u64 JSON                88 u64 file bytes
 *      96 u64 FNV-1a (64 bit) of bytes [0, 96) then [128, end of tables)
 *     104 u64 end of tables: the header, the tables, the descriptors and the
 *         JSON lie below it, the regions' saved bytes from it on
 *     112 .. 127 zero
 *   region table, 32 bytes each: u32 kind (0 arena, 1 saved, 2 zero-filled),
 *       u32 0, u64 bytes, u64 file offset of the saved bytes (0 if none), u64 0.
 *       Region 0 is the plan's arena.  Every region is writable device memory
 *       after load, based on a 256-byte boundary; kinds 0 and 2 start zeroed.
 *   op table, 64 bytes each: u32 OU_OP_* kind, u32 descriptor bytes, u64 file
 *       offset of the descriptor, u32 first relocation, u32 relocation count,
 *       char[40] label (NUL-terminated).  The stored descriptors hold 0 in
 *       every relocated field.
 *   relocation table, 24 bytes each, grouped by op in op order: u32 op,
 *       u32 byte offset in the descriptor (8-byte pointer field), u32 region,
 *       u32 0, u64 offset in the region.
 *   I/O table, 4 entries (mix, noise, out, status) of 32 bytes: u32 region,
 *       u32 count (noise draws; status words; else 0), u64 offset in the
 *       region, u32 batch, u32 samples per item (noise: padded), u64 0.
 *   JSON (UTF-8): fs, n_steps, epsilon, keep_rms, conv_prec, config.
 *
 * Host layer (no HIP call): open validates everything -- versions, every
 * table entry inside the file, descriptor sizes, every relocation inside its
 * descriptor and its region, the lane structure -- so that a file that opens
 * can be materialised at any set of region bases.
 * ---------------------------------------------------------------------- */
typedef struct ou_bundle ou_bundle;
typedef struct ou_model ou_model;

typedef struct ou_bundle_io {
    int32_t region;            /* region the buffer lies in                     */
    int32_t count;             /* noise: draws; status: int32 words; else 0     */
    int64_t offset;            /* byte offset in the region                     */
    int32_t batch;             /* batch items (0 for status)                    */
    int32_t length;            /* samples per item (noise: the padded length)   */
} ou_bundle_io;

typedef struct ou_bundle_meta {
    ou_bundle_io mix;          /* float [batch][length], written by the host    */
    ou_bundle_io noise;        /* float [count][batch][length]                  */
    ou_bundle_io out;          /* float [batch][length], the result             */
    ou_bundle_io status;       /* int32 [count]: [0] GRU hand-off timeout,
                                  [1] and [4..] split-f16 range codes           */
    int32_t n_regions, n_ops;
    int64_t region_bytes;      /* device memory a load allocates, in total      */
    const char* json;          /* NUL-terminated, owned by the handle           */
    int64_t json_bytes;
    char arch[16];
} ou_bundle_meta;

int ou_bundle_open(const char* path, ou_bundle** out);
void ou_bundle_close(ou_bundle* b);
int ou_bundle_info(const ou_bundle* b, ou_bundle_meta* meta);
/* Region i: its kind and size; *data = its saved bytes inside the mapped
 * file (valid until close), NULL for a region that starts zeroed.          */
int ou_bundle_region(const ou_bundle* b, int i, int32_t* kind, int64_t* bytes, const void** data);
/* Op i: its OU_OP_* kind, descriptor size and label (owned by the handle). */
int ou_bundle_op(const ou_bundle* b, int i, int32_t* kind, int64_t* desc_bytes, const char** label);
/* Copy op `op`'s descriptor to desc_out with every relocated field set to
 * region_bases[region] + offset (region_bases: one address per region).    */
int ou_bundle_materialize(const ou_bundle* b, const uint64_t* region_bases, int op, void* desc_out);

/* Device layer: the model-level ABI.  A load allocates every region
 * (hipMalloc), uploads the saved bytes, zeroes the rest, builds the program
 * and, with capture != 0, captures it as one hipGraph; nothing allocates
 * after it.  mix, noise and out are device pointers laid out as
 * ou_bundle_meta describes; the copies in and out and the replay are ordered
 * on ``stream``.  Calls on one handle are not re-entrant.  ou_model_enhance
 * draws the noise with ou_randn (seed, offset) into the noise buffer on the
 * same stream, ahead of the replay and outside the captured graph.
 * ou_model_status waits for the stream last used, reads the status words
 * and zeroes them: 0 clean, 1 GRU hand-off timeout, 2 split-f16 range error
 * (the output is undefined: use a bundle exported with f32 operands),
 * < 0 on a HIP error.                                                       */
int ou_bundle_load(const char* path, int capture, ou_model** out);
int ou_model_enhance_noise(ou_model* m, const float* mix, const float* noise, float* out, void* stream);
int ou_model_enhance(ou_model* m, const float* mix, float* out, uint64_t seed, uint64_t offset, void* stream);
int ou_model_status(ou_model* m);
int ou_model_info(const ou_model* m, ou_bundle_meta* meta);
void ou_model_destroy(ou_model* m);

/* ------------------------------------------------------------------------
 * Windowed enhance of a long clip (ou_long.hip; DESIGN.md section 14 has the
 * definition, open_universe_amd/longform.py restates it on the host).
 *
 * A clip of T samples is cut into n windows of `window` (W) samples that
 * overlap by `overlap` (O) samples, 0 <= O <= W / 2, hop H = W - O:
 *   n = 1 if T == W, else 1 + ceil((T - W) / H);  start(i) = min(i H, T - W)
 * (the last window is shifted back to end at T; nothing is padded), an index
 * i >= n meaning window n - 1.  Window i >= 1 fades in over the O samples
 * [e(i-1) - O, e(i-1)), e(i) = start(i) + W, with weight
 *   f(u) = sin^2(pi (2 u + 1) / (4 O)),  u = t - (e(i-1) - O)
 * while window i - 1 fades out with 1 - f(u); window i has weight 0 before
 * its fade-in, 1 after it until window i + 1 fades in (O = 0: a hard switch
 * at e(i-1)).  At most two windows are non-zero at a sample and the weights
 * sum to 1 on [0, T).  T < W is refused everywhere: such a clip is one plain
 * enhance.
 *
 * ou_long_windows: the arithmetic alone (host; no HIP call): *n and the
 * start of the last window.
 *
 * ou_window_gather: y[r][b][j] = x[r][start(first + b) + j], j < win, for
 * `rows` source rows x_rstride apart and b < count (<= 65535), first < n.
 * win = W for the clip; the sampler's noise uses win = the padded window
 * length, its rows holding start(n - 1) + win values.  x rows must hold
 * T - W + win values; y item b of row r starts at r y_rstride + b y_bstride.
 *
 * ou_overlap_add: adds those of windows [first, first + count) below n (window
 * first + b at w + b w_bstride, W values each), weighted as above, into
 * y[0, T).  fade: [2][O] floats, f(u) then 1 - f(u), rounded from float64
 * (ou_long_fade fills a host array; NULL when O = 0).  The call with
 * first = 0 writes every sample of y (0 where none of its windows is
 * non-zero); a later call adds to what is there.  Products and sums are
 * rounded one by one, so calling it window by window in order, or once, or
 * in any grouping, stores the same bits.
 *
 * All three refuse null pointers, non-positive sizes, O > W / 2, T < W,
 * first < 0 and first >= n.
 * ---------------------------------------------------------------------- */
int ou_long_windows(int64_t T, int window, int overlap, int64_t* n, int64_t* last_start);
int ou_long_fade(int overlap, float* fade /* host, [2][overlap] */);
int ou_window_gather(const float* x, int64_t x_rstride, int rows, int64_t T, int window, int overlap,
                     int64_t first, int count, int64_t win, float* y, int64_t y_rstride, int64_t y_bstride,
                     void* stream);
int ou_overlap_add(const float* w, int64_t w_bstride, int64_t T, int window, int overlap, int64_t first,
                   int count, const float* fade, float* y, void* stream);

/* Pooled windows (ou_pool.hip): the windows of several clips, each longer than
 * W, share the groups of one (B, W) plan.  Clip c of `n_clips` has n_c windows
 * with the starts above; the slot list is every (c, i) in clip order, i
 * ascending, N = sum n_c slots; a group is `count` consecutive slots from slot
 * `first`, a slot index >= N meaning slot N - 1.  The calls keep no state and
 * allocate nothing: each works out its slots from the host array `clips`
 * (device pointers inside) and launches once per 32 slots.
 *
 * ou_pool_slots: the arithmetic alone (host; no HIP call): *n_slots = N.
 *
 * ou_pool_gather: for b < count, slot first + b = (c, i): mix[b mix_bstride + j]
 * = x_c[start_i + j], j < W, and for r < noise_rows: nz[r nz_rstride +
 * b nz_bstride + j] = noise_c[r noise_rstride_c + start_i + j], j < noise_win
 * (the plan's padded window length; a clip's noise rows hold
 * start(n_c - 1) + noise_win values).  One launch per 32 slots copies MIX and
 * every NZ row.  x and, when noise_rows > 0, noise of every clip are read; y is
 * not.
 *
 * ou_pool_overlap_add: crossfades the outputs of slots [first, first + count)
 * below N (slot first + b at w + b w_bstride, W values) into their clips' y.
 * Sample t of a clip belongs to window own = min(t / H, n_c - 1).  The owner
 * stores the finished value, (0 + (1 - f) v_prev) + f v inside its fade-in and
 * 0 + 1 v elsewhere, taking the first term from the previous slot when that is
 * part of this call and from y[t] otherwise; a window whose successor is not
 * part of this call stores 0 + (1 - f) v over the successor's fade-in for the
 * next call to finish.  So the groups must run in slot order from first = 0,
 * after which every sample of every y has been stored (y needs no clearing)
 * with the bits ou_overlap_add gives clip by clip, wherever the group
 * boundaries fall.  y of every clip is written; x and noise are not read.
 *
 * All refuse, on the host: a null list, n_clips < 1, any T <= W, O outside
 * [0, W / 2]; the two launching calls also first outside [0, N), count < 1,
 * null pointers they use, strides smaller than a row, noise_rstride <
 * start(n_c - 1) + noise_win when noise_rows > 0, two clips whose y ranges
 * overlap (overlap_add), and a missing fade table when O > 0 (overlap_add). */
typedef struct ou_pool_clip {      /* host struct, device pointers */
    const float* x;                /* the clip, T samples */
    const float* noise;            /* rows of noise_rstride floats; may be null when noise_rows == 0 */
    float* y;                      /* the result, T samples */
    int64_t T, noise_rstride;
} ou_pool_clip;
int ou_pool_slots(const int64_t* T, int n_clips, int window, int overlap, int64_t* n_slots);
int ou_pool_gather(const ou_pool_clip* clips, int n_clips, int window, int overlap, int64_t first, int count,
                   int noise_rows, int64_t noise_win, float* mix, int64_t mix_bstride,
                   float* nz, int64_t nz_rstride, int64_t nz_bstride, void* stream);
int ou_pool_overlap_add(const ou_pool_clip* clips, int n_clips, int window, int overlap, int64_t first, int count,
                        const float* w, int64_t w_bstride, const float* fade, void* stream);

/* Windowed enhance through a loaded bundle: W and the group size B are the
 * bundle's own (mix.length, mix.batch); x and out are device pointers of n
 * floats, n > W (n <= W is ou_model_enhance's case and refused).  Windows
 * [g B, g B + B) run as one replay each, g = 0, 1, ...: the two kernels
 * above gather the group's windows and noise into the bundle's buffers and
 * overlap-add its output into out, all on ``stream``; unused slots of the
 * last group repeat the last window.  The noise is global: `count` draws
 * (noise.count) of L = start(n - 1) + noise.length values, window i of draw
 * k using noise[k L + start(i) ...), so overlapping windows see the same
 * noise.  ou_model_long_noise returns count L (the floats of that buffer)
 * and, if len is not NULL, L.
 *   _noise: the caller provides the draws, [count][L].
 *   ou_model_enhance_long: draws them with ou_randn into ``workspace``
 *   (caller-owned device memory of ou_model_long_noise floats, free for
 *   reuse when the stream has passed the call): draw k is the stream at
 *   (seed, counter offset + k ceil(L / 4)).
 * Nothing is allocated after load.  The fade table lives in the model and is
 * uploaded when `overlap` differs from the previous call's (that upload
 * waits for the previous call's stream).  ou_model_status is checked once,
 * after the last group, as after ou_model_enhance.                          */
int64_t ou_model_long_noise(const ou_model* m, int64_t n, int overlap, int64_t* len);
int ou_model_enhance_long_noise(ou_model* m, const float* x, int64_t n, int overlap, const float* noise,
                                float* out, void* stream);
int ou_model_enhance_long(ou_model* m, const float* x, int64_t n, int overlap, float* out, uint64_t seed,
                          uint64_t offset, float* workspace, void* stream);

/* ------------------------------------------------------------------------
 * Streaming enhance (ou_stream.hip; DESIGN.md section 15 has the definition,
 * open_universe_amd/longform.py restates the arithmetic on the host).
 *
 * A stream is the windowed enhance above on the concatenation of everything
 * pushed, run as the samples arrive.  With `fed` samples pushed, window i is
 * regular, start i H, and may run as soon as fed >= i H + W; at close, T = fed,
 * the window list is that of a clip of T samples, so only the last window can
 * be shifted, and every window that ran earlier is a regular window of that
 * list.  Windows run in groups [g B, g B + B); the windows left at close run as
 * one last group whose unused slots repeat window n - 1.
 *
 * The noise is a function of position: sample t of draw k is element t of the
 * ou_randn stream at (seed, offset + k 2^38) -- counter offset + k 2^38 +
 * (t >> 2), lane t & 3 -- so it depends neither on T, nor on the grouping, nor
 * on how the pushes were cut; window i uses samples [start(i), start(i) +
 * noise_win) of every draw.  A draw has 2^40 samples: nothing may reach past.
 *
 * The caller keeps an input ring of `cap` >= W floats that holds the samples
 * [lo, fed) of the stream, sample p at ring[p mod cap], and a carry of O
 * floats.  Both calls describe their group as windows [first, first + count)
 * and, with closing != 0, the stream's final length T (first + count must then
 * be the window count of T; the start of the last window is min of its
 * regular start and T - W).
 *
 * ou_stream_gather: for slot b < slots (<= 65535), s_b the start of window
 * first + min(b, count - 1): mix[b mix_bstride + j] = ring[(s_b + j) mod cap],
 * j < W, and for r < noise_rows: nz[r nz_rstride + b nz_bstride + j] = sample
 * s_b + j of draw r, j < noise_win, generated in place with the code of
 * ou_randn (bit-equal to a row of ou_randn sliced at s_b, whatever s_b mod 4
 * is).  One launch per 32 slots.  Refused on the host: null pointers it uses,
 * count < 1, slots < count, O outside [0, W / 2], cap < W, a ring range that
 * is not 0 <= lo <= fed <= lo + cap, a window outside [lo, fed), closing with
 * T != fed or with a window count that is not T's, strides smaller than a row,
 * and noise past sample 2^40.
 *
 * ou_stream_overlap_add: emits the samples the group makes final, out[m] =
 * sample first H + m of the stream for first H + m < (first + count) H, or
 * < T when closing, and stores their number in *n_out (may be NULL).  Sample t
 * belongs to window own = min(t / H, first + count - 1): 0 + 1 v outside the
 * owner's fade-in, (0 + (1 - f) v_prev) + f v inside it, each "+ w v" one fused
 * multiply-add, fma(f, v, fma(1 - f, v_prev, 0)) -- the bits ou_overlap_add
 * gives on the device over the whole stream.  v_prev of
 * window `first` is read from the carry; a call that is not closing then
 * leaves the raw last O samples of window first + count - 1 in the carry.  A
 * closing call with count = 0 -- every window has run and the last one ended
 * at T -- emits the carry alone, with weight 1.  The groups must run in order
 * from first = 0.  w holds window first + b at w + b w_bstride, W values; fade
 * is ou_long_fade's table (NULL when O = 0, and then so may be the carry).  No
 * sample is written twice and nothing needs clearing.  Refused on the host:
 * null pointers it uses, O outside [0, W / 2], count < 1 unless closing,
 * w_bstride < W, and a closing call whose T is shorter than W or does not
 * have first + count windows.
 * ---------------------------------------------------------------------- */
int ou_stream_gather(const float* ring, int64_t cap, int64_t lo, int64_t fed, int window, int overlap, int64_t first,
                     int count, int slots, int closing, int64_t T, int noise_rows, int64_t noise_win, uint64_t seed,
                     uint64_t offset, float* mix, int64_t mix_bstride, float* nz, int64_t nz_rstride,
                     int64_t nz_bstride, void* stream);
int ou_stream_overlap_add(const float* w, int64_t w_bstride, int window, int overlap, int64_t first, int count,
                          int closing, int64_t T, const float* fade, float* carry, float* out, int64_t* n_out,
                          void* stream);

/* A streaming session on a loaded bundle: W and B are the bundle's own; x and
 * out are device pointers.  open allocates the ring (W + B H floats), the carry
 * and the fade table; nothing allocates after it, and the memory does not grow
 * with the stream.  push consumes n >= 0 samples -- any n, in pieces when it is
 * more than the ring has room for -- runs every group that becomes ready
 * (gather, replay, overlap-add, all on ``stream``) and writes the samples they
 * make final to out, *n_out of them: after windows [0, m) have run, samples
 * [0, m H) have been emitted, and the last O samples of window m - 1 wait for
 * their successor.  close runs the windows that are left as one last group and
 * emits everything up to T.  ou_model_stream_bound is the count push(n), or
 * with closing != 0 close, would emit now: host arithmetic on the counts alone,
 * no synchronisation (-1 with a message for a closing stream shorter than W).
 * The concatenated output equals, bit for bit, ou_model_enhance_long_noise on
 * the whole clip with draw k filled by ou_randn at (seed, offset + k 2^38), for
 * every way of cutting the pushes; for T = W, ou_model_enhance_noise on B copies
 * of the window, item 0.
 *
 * close on fewer than W samples fails with OU_STREAM_SHORT; the session stays
 * valid and can be destroyed.  A stream that would pass 2^40 samples is
 * refused.  One session at a time per model: its MIX, NZ and OUT buffers are
 * the model's, so a second open, and every ou_model_enhance* call, is refused
 * while one is open (destroy it first).  Use one stream for all calls of a
 * session, or order them yourself.  ou_model_status applies as after
 * ou_model_enhance: when it reports an error, the session has failed -- the
 * next push or close returns that code and emits nothing.  Destroying the
 * model destroys its open session.                                           */
#define OU_STREAM_SHORT 3
typedef struct ou_stream ou_stream;
int ou_model_stream_open(ou_model* m, int overlap, uint64_t seed, uint64_t offset, ou_stream** out);
int64_t ou_model_stream_bound(const ou_stream* s, int64_t n, int closing);
int ou_model_stream_push(ou_stream* s, const float* x, int64_t n, float* out, int64_t* n_out, void* stream);
int ou_model_stream_close(ou_stream* s, float* out, int64_t* n_out, void* stream);
void ou_model_stream_destroy(ou_stream* s);

/* ------------------------------------------------------------------------
 * Multiplexed streams (ou_mux.hip; DESIGN.md section 16 has the definition,
 * longform.MuxCounts the host arithmetic).
 *
 * C channels are streams as above, each with its own ring, carry, counts and
 * (seed, offset); W, O and H are shared.  The windows that are ready run
 * together in the slots of one batch-B plan: the slot list is [(c, i) for c
 * ascending for i pending in c], group g its slots [g B, g B + B), the unused
 * slots of the last group repeating its last real slot.  The rings are one
 * buffer, channel c's at rings + c cap; the carries one buffer, channel c's at
 * carries + c carry_stride.  Both calls keep no state and allocate nothing.
 *
 * ou_mux_gather: for slot b < n_slots (<= 65535) with channel c, start s and
 * the held range [lo, fed) of c's ring: mix[b mix_bstride + j] = rings[c cap +
 * (s + j) mod cap], j < W, and for r < noise_rows: nz[r nz_rstride + b
 * nz_bstride + j] = sample s + j of draw r of the ou_randn stream at (seed,
 * offset + r 2^38), j < noise_win -- per slot what ou_stream_gather gives for
 * that channel alone, bit for bit.  A padding slot is an ordinary entry that
 * names a window again.  One launch per 32 slots.  Refused on the host: null
 * pointers it uses, n_slots < 1, cap < W, a channel outside [0, channels), a
 * ring range that is not 0 <= lo <= fed <= lo + cap, a window outside [lo,
 * fed), strides smaller than a row, and noise past sample 2^40.
 *
 * ou_mux_overlap_add: a run is a maximal stretch of consecutive slots of one
 * channel in the group, windows [first, first + count) in the slots [slot, slot
 * + count) of w (slot b at w + b w_bstride), with ou_stream_overlap_add's
 * closing and T.  For every run the call emits to out + out_off what
 * ou_stream_overlap_add(w + slot w_bstride, ..., carries + channel
 * carry_stride, out + out_off) emits, bit for bit, and leaves the same carry;
 * n_out[r] (may be NULL) is run r's count.  A run with count = 0 is a closing
 * channel that has nothing left to run: it emits its carry alone.  Slots that
 * belong to no run (padding) are not read, and write nothing.  One launch per
 * 32 runs.  Refused on the host: what ou_stream_overlap_add refuses for a run;
 * n_runs < 1; slots outside [0, n_slots) or not ascending from run to run;
 * channels outside [0, channels) or not strictly ascending (a channel has one
 * run in a group, so no two runs share a carry); outputs that are not ascending
 * without overlap inside [0, out_len); carry_stride < O.
 * ---------------------------------------------------------------------- */
typedef struct ou_mux_slot {
    int64_t start;        /* of the window, in the channel's stream */
    int64_t lo, fed;      /* the channel's ring holds [lo, fed) */
    uint64_t seed, offset;
    int32_t channel, reserved;
} ou_mux_slot;
typedef struct ou_mux_run {
    int64_t first, T;     /* T is read only when closing */
    int64_t out_off;      /* where the run's samples go in out */
    int32_t count, closing;
    int32_t slot;         /* of window `first` in w */
    int32_t channel;
} ou_mux_run;
int ou_mux_gather(const float* rings, int64_t cap, int channels, int window, const ou_mux_slot* slots, int n_slots,
                  int noise_rows, int64_t noise_win, float* mix, int64_t mix_bstride, float* nz, int64_t nz_rstride,
                  int64_t nz_bstride, void* stream);
int ou_mux_overlap_add(const float* w, int64_t w_bstride, int n_slots, int window, int overlap,
                       const ou_mux_run* runs, int n_runs, const float* fade, float* carries, int64_t carry_stride,
                       int channels, float* out, int64_t out_len, int64_t* n_out, void* stream);

/* A mux session on a loaded bundle: W and B are the bundle's own; samples and
 * out are device pointers.  open allocates `channels` rings (W + B H floats
 * each), `channels` carries and the fade table; no device memory is allocated
 * after it, and the memory does not grow with the streams.
 *
 * channel_open takes a free channel (channel < 0: the lowest free one; the
 * index goes to *opened, may be NULL) with its (seed, offset), so a service can
 * reuse channels as calls come and go.  push copies n samples into the
 * channel's ring on ``stream`` and never replays; more than ou_model_mux_room
 * -- cap - (fed - retain), host arithmetic -- is refused whole and consumes
 * nothing: call run first.  close marks the channel closing; on fewer than W
 * samples it fails with OU_STREAM_SHORT for that channel only, which stays
 * open.  A closing channel is free again when run has emitted its last samples.
 *
 * run pools the windows that are ready by the slot rule above, one
 * ou_mux_gather, one replay and one ou_mux_overlap_add per group, all on
 * ``stream``; with full_only != 0 only whole groups run and the rest wait.
 * Channel c's samples land at out + offsets[c], n_out[c] of them (n_out has
 * `channels` entries, may be NULL); ou_model_mux_bound gives those counts and
 * offsets beforehand from the counts alone, no synchronisation, so out can be
 * sized before the call.  Per channel the output is that of an
 * ou_model_stream_* session whose groups are the mux's: y[t] = sum_i
 * weight_i(t) out_i[t - start_i] with out_i what the plan returns for that
 * window in the slot it ran in.
 *
 * One session at a time per model: a mux and a streaming session exclude each
 * other, and every ou_model_enhance* call is refused while a mux is open
 * (destroy it first).  Use one stream for all calls of a session, or order
 * them yourself.  ou_model_status applies as after ou_model_enhance: when it
 * reports an error, or when a run fails, the mux has failed as a whole and
 * every later call returns the code.  Destroying the model destroys its open
 * mux.                                                                       */
typedef struct ou_mux ou_mux;
int ou_model_mux_open(ou_model* m, int overlap, int channels, ou_mux** out);
int ou_model_mux_channel_open(ou_mux* x, int channel, uint64_t seed, uint64_t offset, int* opened);
int64_t ou_model_mux_room(const ou_mux* x, int channel);
int ou_model_mux_push(ou_mux* x, int channel, const float* samples, int64_t n, void* stream);
int ou_model_mux_close(ou_mux* x, int channel);
int ou_model_mux_bound(const ou_mux* x, int full_only, int64_t* counts, int64_t* offsets);
int ou_model_mux_run(ou_mux* x, int full_only, float* out, int64_t* n_out, void* stream);
void ou_model_mux_destroy(ou_mux* x);

#ifdef __cplusplus
}
#endif
#endif /* OUHIP_H */
