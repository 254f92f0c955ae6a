// ou_model.hip -- device layer of the exported enhance bundles: the
// model-level C ABI (include/ouhip.h: ou_bundle_load, ou_model_*).  A load
// gives every region of the file its own hipMalloc (256-byte aligned, as the
// recorder's allocations were), materialises the descriptors at those bases
// into an ou_program and replays it exactly as the recording process did:
// same descriptors, same tiles, same kernels.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/ouhip.h"
#include "ou_common.h"

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

}  // namespace

extern "C" {

void ou_model_destroy(ou_model* m)
{
    if (!m) return;
    (void)hipDeviceSynchronize();   // nothing of it may still run when its memory goes
    if (m->prog) ou_program_destroy(m->prog);
    for (void* p : m->regions)
        if (p) (void)hipFree(p);
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
    hipStream_t s = (hipStream_t)stream;
    int rc = copy_mix(m, mix, s);
    if (rc) return rc;
    if ((rc = ou_randn(m->noise, noise_count(m), seed, offset, stream))) return rc;
    return replay(m, out, s);
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
    if (m->status_host[0]) return ou_fail(1, "GRU recurrence timed out (workgroup hand-off never completed)");
    return ou_fail(2, "split-f16 operand out of range: use a bundle exported with f32 operands");
}

int ou_model_info(const ou_model* m, ou_bundle_meta* meta)
{
    if (!m || !meta) return ou_fail(-1, "model_info: null");
    *meta = m->meta;
    return 0;
}

}  // extern "C"
