// ou_model.hip -- device layer of the exported enhance bundles: the
// model-level C ABI (include/ouhip.h: ou_bundle_load, ou_model_*).  A load
// gives every region of the file its own hipMalloc (256-byte aligned, as the
// recorder's allocations were), materialises the descriptors at those bases
// into an ou_program and replays it exactly as the recording process did:
// same descriptors, same tiles, same kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/ouhip.h"
#include "ou_common.h"

// a streaming session (ou_model_stream_*): the stream's state on the device --
// the input ring, the crossfade carry, the fade table -- and its counts
struct ou_stream {
    ou_model* m = nullptr;
    int W = 0, B = 0, Tp = 0, O = 0, rows = 0;
    long long H = 0, cap = 0;
    uint64_t seed = 0, offset = 0;
    long long fed = 0, run = 0;   // samples pushed; windows run, a multiple of B until close
    bool closed = false;
    int failed = 0;               // the code ou_model_status reported: every later call returns it
    float *ring = nullptr, *carry = nullptr, *fade = nullptr;
};

// a mux session (ou_model_mux_*): `C` channels, each a stream of its own -- ring c at rings + c cap, carry c at
// carries + c cs -- whose ready windows share the slots of the model's plan
struct ou_mux_channel {
    int state = 0;                // 0 free, 1 open, 2 closing
    long long fed = 0, run = 0;
    uint64_t seed = 0, offset = 0;
};

struct ou_mux {
    ou_model* m = nullptr;
    int W = 0, B = 0, Tp = 0, O = 0, rows = 0, C = 0;
    long long H = 0, cap = 0, cs = 0;
    int failed = 0;               // a failed call's code, or what ou_model_status reported: every later call returns it
    std::vector<ou_mux_channel> ch;
    float *rings = nullptr, *carries = nullptr, *fade = nullptr;
};

struct ou_model {
    ou_bundle* bundle = nullptr;
    ou_bundle_meta meta{};
    std::vector<void*> regions;
    ou_program* prog = nullptr;
    bool captured = false;
    float *mix = nullptr, *noise = nullptr, *out = nullptr;
    int32_t* status = nullptr;
    std::vector<int32_t> status_host;
    hipStream_t last = nullptr;   // the stream of the latest enhance: ou_model_status waits for it
    // windowed enhance (ou_model_enhance_long*): the crossfade table [2][overlap] for the
    // overlap of the latest call, in a buffer of mix.length floats allocated at load
    float* fade = nullptr;
    int fade_overlap = -1;
    std::vector<float> fade_host;
    ou_stream* live = nullptr;   // the open streaming session: it owns mix, noise and out until destroyed
    ou_mux* mux = nullptr;       // or the open mux session: the two exclude each other
};

namespace {

void* io_ptr(const ou_model* m, const ou_bundle_io& io) { return (char*)m->regions[io.region] + io.offset; }

int build(ou_model* m, const char* path, int capture)
{
    int rc = ou_bundle_open(path, &m->bundle);
    if (rc) return rc;
    if ((rc = ou_bundle_info(m->bundle, &m->meta))) return rc;
    const int nr = m->meta.n_regions;
    m->regions.assign(nr, nullptr);
    std::vector<uint64_t> bases(nr, 0);
    for (int i = 0; i < nr; ++i) {
        int32_t kind = 0;
        int64_t bytes = 0;
        const void* data = nullptr;
        if ((rc = ou_bundle_region(m->bundle, i, &kind, &bytes, &data))) return rc;
        OU_HIP_CHECK(hipMalloc(&m->regions[i], (size_t)bytes), "bundle_load: region allocation");
        if ((uintptr_t)m->regions[i] % 256) return ou_fail(-1, "bundle_load: region %d is not 256-byte aligned", i);
        if (data) OU_HIP_CHECK(hipMemcpy(m->regions[i], data, (size_t)bytes, hipMemcpyHostToDevice), "bundle_load: upload");
        else OU_HIP_CHECK(hipMemset(m->regions[i], 0, (size_t)bytes), "bundle_load: zero fill");
        bases[i] = (uint64_t)(uintptr_t)m->regions[i];
    }
    m->prog = ou_program_create();
    std::vector<unsigned char> desc;
    for (int i = 0; i < m->meta.n_ops; ++i) {
        int32_t kind = 0;
        int64_t bytes = 0;
        if ((rc = ou_bundle_op(m->bundle, i, &kind, &bytes, nullptr))) return rc;
        desc.assign((size_t)bytes, 0);
        if ((rc = ou_bundle_materialize(m->bundle, bases.data(), i, desc.data()))) return rc;
        if ((rc = ou_program_add(m->prog, kind, desc.data(), desc.size()))) return rc;
    }
    if ((rc = ou_program_validate(m->prog))) return rc;
    m->mix = (float*)io_ptr(m, m->meta.mix);
    m->noise = (float*)io_ptr(m, m->meta.noise);
    m->out = (float*)io_ptr(m, m->meta.out);
    m->status = (int32_t*)io_ptr(m, m->meta.status);
    m->status_host.assign(m->meta.status.count, 0);
    OU_HIP_CHECK(hipMalloc((void**)&m->fade, 4ull * (size_t)m->meta.mix.length), "bundle_load: fade table");
    OU_HIP_CHECK(hipDeviceSynchronize(), "bundle_load: sync");   // the uploads and fills, before any stream uses them
    if (capture) {
        if ((rc = ou_program_capture(m->prog))) return rc;
        m->captured = true;
    }
    return 0;
}

int replay(ou_model* m, float* out, hipStream_t s)
{
    const int rc = m->captured ? ou_program_launch(m->prog, s) : ou_program_run(m->prog, s);
    if (rc) return rc;
    const size_t n = 4ull * m->meta.out.batch * m->meta.out.length;
    OU_HIP_CHECK(hipMemcpyAsync(out, m->out, n, hipMemcpyDeviceToDevice, s), "model_enhance: copy out");
    return 0;
}

int copy_mix(ou_model* m, const float* mix, hipStream_t s)
{
    const size_t n = 4ull * m->meta.mix.batch * m->meta.mix.length;
    OU_HIP_CHECK(hipMemcpyAsync(m->mix, mix, n, hipMemcpyDeviceToDevice, s), "model_enhance: copy mix");
    m->last = s;
    return 0;
}

int64_t noise_count(const ou_model* m)
{
    return (int64_t)m->meta.noise.count * m->meta.noise.batch * m->meta.noise.length;
}

// the windowed enhance's geometry for a clip of n samples: the window count
// and L, the length of one global noise draw
int long_check(const ou_model* m, const char* what, int64_t n, int overlap, int64_t* n_win, int64_t* len)
{
    const int W = m->meta.mix.length;
    if (n <= W) return ou_fail(-1, "%s: a clip of %lld samples fits one window of %d: use ou_model_enhance", what,
                               (long long)n, W);
    int64_t last = 0;
    const int rc = ou_long_windows(n, W, overlap, n_win, &last);
    if (rc) return rc;
    *len = last + m->meta.noise.length;
    return 0;
}

int long_fade(ou_model* m, int overlap, hipStream_t s)
{
    if (overlap == m->fade_overlap) return 0;
    // the previous call's overlap-adds may still read the table
    OU_HIP_CHECK(hipStreamSynchronize(m->last), "model_enhance_long: sync");
    if (s != m->last) OU_HIP_CHECK(hipStreamSynchronize(s), "model_enhance_long: sync");
    m->fade_host.assign(2 * (size_t)overlap + 1, 0.f);
    const int rc = ou_long_fade(overlap, m->fade_host.data());
    if (rc) return rc;
    if (overlap > 0)
        OU_HIP_CHECK(hipMemcpy(m->fade, m->fade_host.data(), 8ull * overlap, hipMemcpyHostToDevice),
                     "model_enhance_long: fade table");
    m->fade_overlap = overlap;
    return 0;
}

// groups of `batch` windows: gather, replay, overlap-add, all on s
int long_run(ou_model* m, const float* x, int64_t n, int overlap, const float* noise, int64_t n_win, int64_t len,
             float* out, hipStream_t s)
{
    const int W = m->meta.mix.length, B = m->meta.mix.batch, Tp = m->meta.noise.length;
    int rc = long_fade(m, overlap, s);
    if (rc) return rc;
    m->last = s;
    for (int64_t first = 0; first < n_win; first += B) {
        if ((rc = ou_window_gather(x, 0, 1, n, W, overlap, first, B, W, m->mix, 0, W, s))) return rc;
        if (m->meta.noise.count > 0 &&
            (rc = ou_window_gather(noise, len, m->meta.noise.count, n, W, overlap, first, B, Tp, m->noise,
                                   (int64_t)B * Tp, Tp, s)))
            return rc;
        if ((rc = m->captured ? ou_program_launch(m->prog, s) : ou_program_run(m->prog, s))) return rc;
        if ((rc = ou_overlap_add(m->out, W, n, W, overlap, first, B, overlap > 0 ? m->fade : nullptr, out, s)))
            return rc;
    }
    return 0;
}

constexpr long long kStreamMaxSamples = 1LL << 40;

// windows of a stream that are regular and whose samples are all there
long long stream_ready(const ou_stream* s, long long fed) { return fed < s->W ? 0 : (fed - s->W) / s->H + 1; }

// windows [first, first + count) as one group: gather, replay, overlap-add, all on st
int stream_group(ou_stream* s, long long first, int count, int closing, float* out, int64_t* n_out, hipStream_t st)
{
    ou_model* m = s->m;
    const long long lo = s->fed > s->cap ? s->fed - s->cap : 0;
    int rc = 0;
    if (count > 0) {
        if ((rc = ou_stream_gather(s->ring, s->cap, lo, s->fed, s->W, s->O, first, count, s->B, closing, s->fed,
                                   s->rows, s->Tp, s->seed, s->offset, m->mix, s->W, m->noise,
                                   (int64_t)s->B * s->Tp, s->Tp, st)))
            return rc;
        if ((rc = m->captured ? ou_program_launch(m->prog, st) : ou_program_run(m->prog, st))) return rc;
    }
    return ou_stream_overlap_add(m->out, s->W, s->W, s->O, first, count, closing, s->fed,
                                 s->O > 0 ? s->fade : nullptr, s->carry, out, n_out, st);
}

int stream_usable(const ou_stream* s, const char* what)
{
    if (s->failed) return ou_fail(s->failed, "%s: the session failed (ou_model_status reported %d)", what, s->failed);
    if (s->closed) return ou_fail(-1, "%s: the session is closed", what);
    return 0;
}

// ---- the mux session's host arithmetic (longform.MuxCounts states it in Python)
long long mux_windows(const ou_mux* x, long long T) { return T <= x->W ? 1 : 1 + (T - x->W + x->H - 1) / x->H; }

// the windows of channel c that can run now: [run, *stop)
long long mux_pending_stop(const ou_mux* x, int c)
{
    const ou_mux_channel& s = x->ch[c];
    if (s.state == 0) return s.run;
    if (s.state == 2) return mux_windows(x, s.fed);
    return s.fed < x->W ? 0 : (s.fed - x->W) / x->H + 1;
}

long long mux_room(const ou_mux* x, int c)
{
    const ou_mux_channel& s = x->ch[c];
    long long keep = s.run * x->H < s.fed - x->W ? s.run * x->H : s.fed - x->W;
    if (keep < 0) keep = 0;
    return s.state == 1 ? x->cap - (s.fed - keep) : 0;
}

struct MuxGroup {
    std::vector<ou_mux_slot> slots;   // B of them, or none
    std::vector<ou_mux_run> runs;
};
struct MuxPlan {
    std::vector<MuxGroup> groups;
    std::vector<int64_t> counts, offsets, after;   // per channel: samples emitted, where, windows run afterwards
    std::vector<int> freed;
};

// what run(full_only) does now: the slot list [(c, i) for c ascending for i pending in c] in groups of B, the
// unused slots of the last group repeating its last real slot; a run is a maximal stretch of one channel's slots in
// a group; a closing channel with nothing left to run is a run without slots and goes with the first group
void mux_plan(const ou_mux* x, int full_only, MuxPlan* p)
{
    const int C = x->C, B = x->B;
    const long long H = x->H;
    struct Slot {
        int c;
        long long i;
    };
    std::vector<Slot> S;
    for (int c = 0; c < C; ++c)
        for (long long i = x->ch[c].run, stop = mux_pending_stop(x, c); i < stop; ++i) S.push_back({c, i});
    if (full_only) S.resize(S.size() / B * B);
    p->counts.assign(C, 0), p->offsets.assign(C, 0), p->after.assign(C, 0);
    for (int c = 0; c < C; ++c) p->after[c] = x->ch[c].run;
    std::vector<ou_mux_run> alone;
    for (int c = 0; c < C; ++c) {
        const ou_mux_channel& s = x->ch[c];
        if (s.state == 2 && s.run == mux_windows(x, s.fed)) {
            alone.push_back({s.run, s.fed, 0, 0, 1, 0, c});
            p->counts[c] = s.fed - s.run * H;
            p->freed.push_back(c);
        }
    }
    for (size_t g = 0; g < S.size(); g += B) {
        MuxGroup G;
        const size_t stop = g + B < S.size() ? g + B : S.size();
        for (size_t b = g; b < g + B; ++b) {
            const Slot& e = S[b < stop ? b : stop - 1];
            const ou_mux_channel& s = x->ch[e.c];
            long long start = e.i * H;
            if (s.state == 2 && start > s.fed - x->W) start = s.fed - x->W;
            G.slots.push_back({start, s.fed > x->cap ? s.fed - x->cap : 0, s.fed, s.seed, s.offset, e.c, 0});
            if (b >= stop) continue;
            if (!G.runs.empty() && G.runs.back().channel == e.c) ++G.runs.back().count;
            else G.runs.push_back({e.i, 0, 0, 1, 0, (int32_t)(b - g), e.c});
        }
        for (ou_mux_run& r : G.runs) {
            const ou_mux_channel& s = x->ch[r.channel];
            const long long last = r.first + r.count;
            if (s.state == 2 && last == mux_windows(x, s.fed)) {
                r.closing = 1, r.T = s.fed;
                p->freed.push_back(r.channel);
            }
            p->counts[r.channel] += (r.closing ? s.fed : last * H) - r.first * H;
            p->after[r.channel] = last;
        }
        p->groups.push_back(std::move(G));
    }
    if (!alone.empty()) {
        if (p->groups.empty()) p->groups.emplace_back();
        std::vector<ou_mux_run>& r = p->groups[0].runs;
        r.insert(r.end(), alone.begin(), alone.end());
        std::sort(r.begin(), r.end(), [](const ou_mux_run& a, const ou_mux_run& b) { return a.channel < b.channel; });
    }
    for (int c = 1; c < C; ++c) p->offsets[c] = p->offsets[c - 1] + p->counts[c - 1];
    std::vector<int64_t> at = p->offsets;
    for (MuxGroup& G : p->groups)
        for (ou_mux_run& r : G.runs) {
            r.out_off = at[r.channel];
            at[r.channel] += (r.closing ? r.T : (r.first + r.count) * H) - r.first * H;
        }
}

int mux_usable(const ou_mux* x, const char* what)
{
    if (x->failed) return ou_fail(x->failed, "%s: the mux failed earlier (code %d)", what, x->failed);
    return 0;
}

int mux_channel(const ou_mux* x, int c, const char* what)
{
    if (c < 0 || c >= x->C) return ou_fail(-1, "%s: channel %d of %d", what, c, x->C);
    if (x->ch[c].state == 0) return ou_fail(-1, "%s: channel %d is free", what, c);
    return 0;
}

}  // namespace

extern "C" {

void ou_model_destroy(ou_model* m)
{
    if (!m) return;
    if (m->live) ou_model_stream_destroy(m->live);
    if (m->mux) ou_model_mux_destroy(m->mux);
    (void)hipDeviceSynchronize();   // nothing of it may still run when its memory goes
    if (m->prog) ou_program_destroy(m->prog);
    for (void* p : m->regions)
        if (p) (void)hipFree(p);
    if (m->fade) (void)hipFree(m->fade);
    if (m->bundle) ou_bundle_close(m->bundle);
    delete m;
}

int ou_bundle_load(const char* path, int capture, ou_model** out)
{
    if (!path || !out) return ou_fail(-1, "bundle_load: null");
    *out = nullptr;
    ou_model* m = new ou_model();
    const int rc = build(m, path, capture);
    if (rc) {
        ou_model_destroy(m);   // keeps the message ou_fail left
        return rc;
    }
    *out = m;
    return 0;
}

int ou_model_enhance_noise(ou_model* m, const float* mix, const float* noise, float* out, void* stream)
{
    if (!m || !mix || !noise || !out) return ou_fail(-1, "model_enhance_noise: null");
    if (m->live) return ou_fail(-1, "model_enhance_noise: a streaming session is open on this model");
    if (m->mux) return ou_fail(-1, "model_enhance_noise: a mux session is open on this model");
    hipStream_t s = (hipStream_t)stream;
    int rc = copy_mix(m, mix, s);
    if (rc) return rc;
    OU_HIP_CHECK(hipMemcpyAsync(m->noise, noise, 4ull * noise_count(m), hipMemcpyDeviceToDevice, s),
                 "model_enhance_noise: copy noise");
    return replay(m, out, s);
}

int ou_model_enhance(ou_model* m, const float* mix, float* out, uint64_t seed, uint64_t offset, void* stream)
{
    if (!m || !mix || !out) return ou_fail(-1, "model_enhance: null");
    if (m->live) return ou_fail(-1, "model_enhance: a streaming session is open on this model");
    if (m->mux) return ou_fail(-1, "model_enhance: a mux session is open on this model");
    hipStream_t s = (hipStream_t)stream;
    int rc = copy_mix(m, mix, s);
    if (rc) return rc;
    if ((rc = ou_randn(m->noise, noise_count(m), seed, offset, stream))) return rc;
    return replay(m, out, s);
}

int64_t ou_model_long_noise(const ou_model* m, int64_t n, int overlap, int64_t* len)
{
    if (!m) return ou_fail(-1, "model_long_noise: null");
    int64_t n_win = 0, l = 0;
    const int rc = long_check(m, "model_long_noise", n, overlap, &n_win, &l);
    if (rc) return rc;
    if (len) *len = l;
    return (int64_t)m->meta.noise.count * l;
}

int ou_model_enhance_long_noise(ou_model* m, const float* x, int64_t n, int overlap, const float* noise,
                                float* out, void* stream)
{
    if (!m || !x || !noise || !out) return ou_fail(-1, "model_enhance_long_noise: null");
    if (m->live) return ou_fail(-1, "model_enhance_long_noise: a streaming session is open on this model");
    if (m->mux) return ou_fail(-1, "model_enhance_long_noise: a mux session is open on this model");
    int64_t n_win = 0, len = 0;
    const int rc = long_check(m, "model_enhance_long_noise", n, overlap, &n_win, &len);
    if (rc) return rc;
    return long_run(m, x, n, overlap, noise, n_win, len, out, (hipStream_t)stream);
}

int ou_model_enhance_long(ou_model* m, const float* x, int64_t n, int overlap, float* out, uint64_t seed,
                          uint64_t offset, float* workspace, void* stream)
{
    if (!m || !x || !out || !workspace) return ou_fail(-1, "model_enhance_long: null");
    if (m->live) return ou_fail(-1, "model_enhance_long: a streaming session is open on this model");
    if (m->mux) return ou_fail(-1, "model_enhance_long: a mux session is open on this model");
    int64_t n_win = 0, len = 0;
    int rc = long_check(m, "model_enhance_long", n, overlap, &n_win, &len);
    if (rc) return rc;
    const uint64_t per_draw = (uint64_t)((len + 3) / 4);
    for (int k = 0; k < m->meta.noise.count; ++k)
        if ((rc = ou_randn(workspace + (int64_t)k * len, len, seed, offset + (uint64_t)k * per_draw, stream))) return rc;
    return long_run(m, x, n, overlap, workspace, n_win, len, out, (hipStream_t)stream);
}

int ou_model_status(ou_model* m)
{
    if (!m) return ou_fail(-1, "model_status: null");
    OU_HIP_CHECK(hipStreamSynchronize(m->last), "model_status: sync");
    const size_t n = 4 * m->status_host.size();
    OU_HIP_CHECK(hipMemcpy(m->status_host.data(), m->status, n, hipMemcpyDeviceToHost), "model_status: read");
    bool any = false;
    for (int32_t w : m->status_host) any = any || w;
    if (!any) return 0;
    OU_HIP_CHECK(hipMemsetAsync(m->status, 0, n, m->last), "model_status: clear");
    OU_HIP_CHECK(hipStreamSynchronize(m->last), "model_status: sync");
    if (m->live) m->live->failed = m->status_host[0] ? 1 : 2;
    if (m->mux) m->mux->failed = m->status_host[0] ? 1 : 2;
    if (m->status_host[0]) return ou_fail(1, "GRU recurrence timed out (workgroup hand-off never completed)");
    return ou_fail(2, "split-f16 operand out of range: use a bundle exported with f32 operands");
}

int ou_model_info(const ou_model* m, ou_bundle_meta* meta)
{
    if (!m || !meta) return ou_fail(-1, "model_info: null");
    *meta = m->meta;
    return 0;
}

int ou_model_stream_open(ou_model* m, int overlap, uint64_t seed, uint64_t offset, ou_stream** out)
{
    if (!m || !out) return ou_fail(-1, "model_stream_open: null");
    *out = nullptr;
    if (m->live) return ou_fail(-1, "model_stream_open: a streaming session is already open on this model");
    if (m->mux) return ou_fail(-1, "model_stream_open: a mux session is open on this model");
    const int W = m->meta.mix.length;
    if (overlap < 0 || overlap > W / 2)
        return ou_fail(-1, "model_stream_open: overlap %d outside [0, window / 2] = [0, %d]", overlap, W / 2);
    ou_stream* s = new ou_stream();
    s->m = m;
    s->W = W, s->B = m->meta.mix.batch, s->Tp = m->meta.noise.length, s->O = overlap, s->rows = m->meta.noise.count;
    s->H = W - overlap;
    s->cap = W + s->B * s->H;
    s->seed = seed, s->offset = offset;
    std::vector<float> tab(2 * (size_t)overlap + 1, 0.f);
    int rc = ou_long_fade(overlap, tab.data());
    hipError_t e = hipSuccess;
    if (!rc && (e = hipMalloc((void**)&s->ring, 4ull * (size_t)s->cap)) != hipSuccess) rc = -1;
    if (!rc && (e = hipMalloc((void**)&s->carry, 4ull * (size_t)(overlap + 1))) != hipSuccess) rc = -1;
    if (!rc && (e = hipMalloc((void**)&s->fade, 4ull * (2 * (size_t)overlap + 1))) != hipSuccess) rc = -1;
    if (!rc && (e = hipMemcpy(s->fade, tab.data(), 4ull * (2 * (size_t)overlap + 1), hipMemcpyHostToDevice)) != hipSuccess)
        rc = -1;
    if (rc) {
        if (e != hipSuccess) ou_fail(-1, "model_stream_open: %s", hipGetErrorString(e));
        ou_model_stream_destroy(s);
        return rc;
    }
    m->live = s;
    *out = s;
    return 0;
}

int64_t ou_model_stream_bound(const ou_stream* s, int64_t n, int closing)
{
    if (!s || n < 0) return ou_fail(-1, "model_stream_bound: bad arguments");
    if (s->failed || s->closed) return 0;
    if (closing) {
        if (s->fed < s->W)
            return ou_fail(-1, "model_stream_bound: a stream of %lld samples is shorter than one window of %d",
                           s->fed, s->W);
        return s->fed - s->run * s->H;
    }
    const long long ready = stream_ready(s, s->fed + n);
    return (ready - s->run) / s->B * s->B * s->H;
}

int ou_model_stream_push(ou_stream* s, const float* x, int64_t n, float* out, int64_t* n_out, void* stream)
{
    if (!s || n < 0 || (n > 0 && !x)) return ou_fail(-1, "model_stream_push: bad arguments");
    if (n_out) *n_out = 0;
    int rc = stream_usable(s, "model_stream_push");
    if (rc) return rc;
    if (s->fed + n + (s->Tp - s->W) > kStreamMaxSamples)
        return ou_fail(-1, "model_stream_push: the stream would pass 2^40 samples");
    if (ou_model_stream_bound(s, n, 0) > 0 && !out) return ou_fail(-1, "model_stream_push: null output");
    hipStream_t st = (hipStream_t)stream;
    s->m->last = st;
    long long left = n, total = 0;
    for (;;) {
        while (stream_ready(s, s->fed) - s->run >= s->B) {
            int64_t got = 0;
            if ((rc = stream_group(s, s->run, s->B, 0, out + total, &got, st))) return rc;
            s->run += s->B;
            total += got;
            if (n_out) *n_out = total;
        }
        if (left == 0) break;
        // the ring keeps [min(run H, fed - W), fed): the next window's samples, and the last W for a shifted close
        long long keep = s->run * s->H < s->fed - s->W ? s->run * s->H : s->fed - s->W;
        if (keep < 0) keep = 0;
        const long long room = s->cap - (s->fed - keep);
        if (room <= 0) return ou_fail(-1, "model_stream_push: the ring is full with no group ready");
        const long long take = left < room ? left : room;
        const long long at = s->fed % s->cap;
        const long long head = take < s->cap - at ? take : s->cap - at;
        OU_HIP_CHECK(hipMemcpyAsync(s->ring + at, x, 4ull * (size_t)head, hipMemcpyDeviceToDevice, st),
                     "model_stream_push: copy in");
        if (take > head)
            OU_HIP_CHECK(hipMemcpyAsync(s->ring, x + head, 4ull * (size_t)(take - head), hipMemcpyDeviceToDevice, st),
                         "model_stream_push: copy in");
        s->fed += take, x += take, left -= take;
    }
    return 0;
}

int ou_model_stream_close(ou_stream* s, float* out, int64_t* n_out, void* stream)
{
    if (!s) return ou_fail(-1, "model_stream_close: null");
    if (n_out) *n_out = 0;
    int rc = stream_usable(s, "model_stream_close");
    if (rc) return rc;
    if (s->fed < s->W)
        return ou_fail(OU_STREAM_SHORT, "model_stream_close: a stream of %lld samples is shorter than one window of %d",
                       s->fed, s->W);
    const long long n = 1 + (s->fed - s->W + s->H - 1) / s->H;
    if (s->fed - s->run * s->H > 0 && !out) return ou_fail(-1, "model_stream_close: null output");
    s->m->last = (hipStream_t)stream;
    if ((rc = stream_group(s, s->run, (int)(n - s->run), 1, out, n_out, (hipStream_t)stream))) return rc;
    s->run = n;
    s->closed = true;
    return 0;
}

void ou_model_stream_destroy(ou_stream* s)
{
    if (!s) return;
    (void)hipDeviceSynchronize();   // nothing of it may still run when its memory goes
    if (s->ring) (void)hipFree(s->ring);
    if (s->carry) (void)hipFree(s->carry);
    if (s->fade) (void)hipFree(s->fade);
    if (s->m && s->m->live == s) s->m->live = nullptr;
    delete s;
}

int ou_model_mux_open(ou_model* m, int overlap, int channels, ou_mux** out)
{
    if (!m || !out) return ou_fail(-1, "model_mux_open: null");
    *out = nullptr;
    if (m->live) return ou_fail(-1, "model_mux_open: a streaming session is open on this model");
    if (m->mux) return ou_fail(-1, "model_mux_open: a mux session is already open on this model");
    const int W = m->meta.mix.length;
    if (overlap < 0 || overlap > W / 2)
        return ou_fail(-1, "model_mux_open: overlap %d outside [0, window / 2] = [0, %d]", overlap, W / 2);
    if (channels < 1 || channels > 65535) return ou_fail(-1, "model_mux_open: %d channels", channels);
    ou_mux* x = new ou_mux();
    x->m = m;
    x->W = W, x->B = m->meta.mix.batch, x->Tp = m->meta.noise.length, x->O = overlap, x->rows = m->meta.noise.count;
    x->C = channels;
    x->H = W - overlap;
    x->cap = W + x->B * x->H;
    x->cs = overlap > 0 ? overlap : 1;
    x->ch.assign((size_t)channels, ou_mux_channel());
    std::vector<float> tab(2 * (size_t)overlap + 1, 0.f);
    int rc = ou_long_fade(overlap, tab.data());
    hipError_t e = hipSuccess;
    if (!rc && (e = hipMalloc((void**)&x->rings, 4ull * (size_t)x->cap * channels)) != hipSuccess) rc = -1;
    if (!rc && (e = hipMalloc((void**)&x->carries, 4ull * (size_t)x->cs * channels)) != hipSuccess) rc = -1;
    if (!rc && (e = hipMalloc((void**)&x->fade, 4ull * (2 * (size_t)overlap + 1))) != hipSuccess) rc = -1;
    if (!rc && (e = hipMemcpy(x->fade, tab.data(), 4ull * (2 * (size_t)overlap + 1), hipMemcpyHostToDevice)) != hipSuccess)
        rc = -1;
    if (rc) {
        if (e != hipSuccess) ou_fail(-1, "model_mux_open: %s", hipGetErrorString(e));
        ou_model_mux_destroy(x);
        return rc;
    }
    m->mux = x;
    *out = x;
    return 0;
}

int ou_model_mux_channel_open(ou_mux* x, int channel, uint64_t seed, uint64_t offset, int* opened)
{
    if (!x) return ou_fail(-1, "model_mux_channel_open: null");
    int rc = mux_usable(x, "model_mux_channel_open");
    if (rc) return rc;
    if (channel < 0) {
        for (channel = 0; channel < x->C && x->ch[channel].state != 0; ++channel) {}
        if (channel == x->C) return ou_fail(-1, "model_mux_channel_open: all %d channels are busy", x->C);
    }
    if (channel >= x->C) return ou_fail(-1, "model_mux_channel_open: channel %d of %d", channel, x->C);
    ou_mux_channel& s = x->ch[channel];
    if (s.state != 0)
        return ou_fail(-1, "model_mux_channel_open: channel %d is %s", channel, s.state == 1 ? "open" : "closing");
    s = ou_mux_channel();
    s.state = 1, s.seed = seed, s.offset = offset;
    if (opened) *opened = channel;
    return 0;
}

int64_t ou_model_mux_room(const ou_mux* x, int channel)
{
    if (!x) return ou_fail(-1, "model_mux_room: null");
    const int rc = mux_channel(x, channel, "model_mux_room");
    return rc ? rc : mux_room(x, channel);
}

int ou_model_mux_push(ou_mux* x, int channel, const float* samples, int64_t n, void* stream)
{
    if (!x || n < 0 || (n > 0 && !samples)) return ou_fail(-1, "model_mux_push: bad arguments");
    int rc = mux_usable(x, "model_mux_push");
    if (rc || (rc = mux_channel(x, channel, "model_mux_push"))) return rc;
    ou_mux_channel& s = x->ch[channel];
    if (s.state != 1) return ou_fail(-1, "model_mux_push: channel %d is closing", channel);
    if (n > mux_room(x, channel))
        return ou_fail(-1, "model_mux_push: %lld samples, channel %d has room for %lld: run first", (long long)n,
                       channel, mux_room(x, channel));
    if (s.fed + n + (x->Tp - x->W) > kStreamMaxSamples)
        return ou_fail(-1, "model_mux_push: the stream would pass 2^40 samples");
    hipStream_t st = (hipStream_t)stream;
    float* ring = x->rings + (long long)channel * x->cap;
    const long long at = s.fed % x->cap;
    const long long head = n < x->cap - at ? n : x->cap - at;
    if (head > 0)
        OU_HIP_CHECK(hipMemcpyAsync(ring + at, samples, 4ull * (size_t)head, hipMemcpyDeviceToDevice, st),
                     "model_mux_push: copy in");
    if (n > head)
        OU_HIP_CHECK(hipMemcpyAsync(ring, samples + head, 4ull * (size_t)(n - head), hipMemcpyDeviceToDevice, st),
                     "model_mux_push: copy in");
    s.fed += n;
    return 0;
}

int ou_model_mux_close(ou_mux* x, int channel)
{
    if (!x) return ou_fail(-1, "model_mux_close: null");
    int rc = mux_usable(x, "model_mux_close");
    if (rc || (rc = mux_channel(x, channel, "model_mux_close"))) return rc;
    ou_mux_channel& s = x->ch[channel];
    if (s.state != 1) return ou_fail(-1, "model_mux_close: channel %d is closing", channel);
    if (s.fed < x->W)
        return ou_fail(OU_STREAM_SHORT, "model_mux_close: channel %d: a stream of %lld samples is shorter than one "
                       "window of %d", channel, s.fed, x->W);
    s.state = 2;
    return 0;
}

int ou_model_mux_bound(const ou_mux* x, int full_only, int64_t* counts, int64_t* offsets)
{
    if (!x) return ou_fail(-1, "model_mux_bound: null");
    MuxPlan p;
    if (!x->failed) mux_plan(x, full_only, &p);
    for (int c = 0; c < x->C; ++c) {
        if (counts) counts[c] = x->failed ? 0 : p.counts[c];
        if (offsets) offsets[c] = x->failed ? 0 : p.offsets[c];
    }
    return 0;
}

int ou_model_mux_run(ou_mux* x, int full_only, float* out, int64_t* n_out, void* stream)
{
    if (!x) return ou_fail(-1, "model_mux_run: null");
    if (n_out)
        for (int c = 0; c < x->C; ++c) n_out[c] = 0;
    int rc = mux_usable(x, "model_mux_run");
    if (rc) return rc;
    MuxPlan p;
    mux_plan(x, full_only, &p);
    const int64_t total = p.offsets[x->C - 1] + p.counts[x->C - 1];
    if (total > 0 && !out) return ou_fail(-1, "model_mux_run: null output");
    ou_model* m = x->m;
    hipStream_t st = (hipStream_t)stream;
    m->last = st;
    for (const MuxGroup& G : p.groups) {
        const int ns = (int)G.slots.size();
        if (ns > 0) {
            rc = ou_mux_gather(x->rings, x->cap, x->C, x->W, G.slots.data(), ns, x->rows, x->Tp, m->mix, x->W,
                               m->noise, (int64_t)x->B * x->Tp, x->Tp, st);
            if (!rc) rc = m->captured ? ou_program_launch(m->prog, st) : ou_program_run(m->prog, st);
        }
        if (!rc)
            rc = ou_mux_overlap_add(m->out, x->W, ns, x->W, x->O, G.runs.data(), (int)G.runs.size(),
                                    x->O > 0 ? x->fade : nullptr, x->O > 0 ? x->carries : nullptr, x->cs, x->C, out,
                                    total, nullptr, st);
        if (rc) {   // the counts would run ahead of the device: the mux fails as a whole
            x->failed = rc;
            return rc;
        }
    }
    for (int c = 0; c < x->C; ++c) {
        x->ch[c].run = p.after[c];
        if (n_out) n_out[c] = p.counts[c];
    }
    for (int c : p.freed) x->ch[c] = ou_mux_channel();
    return 0;
}

void ou_model_mux_destroy(ou_mux* x)
{
    if (!x) return;
    (void)hipDeviceSynchronize();   // nothing of it may still run when its memory goes
    if (x->rings) (void)hipFree(x->rings);
    if (x->carries) (void)hipFree(x->carries);
    if (x->fade) (void)hipFree(x->fade);
    if (x->m && x->m->mux == x) x->m->mux = nullptr;
    delete x;
}

}  // extern "C"
