// enhance_host.cpp -- enhance one clip from a C++ host, without Python: load
// an exported bundle (python -m open_universe_amd.bin.export_bundle), feed it
// raw little-endian float32 samples, write the result the same way.
//
//   enhance_host BUNDLE.oub MIX.f32 OUT.f32 [NOISE.f32 | --seed N]
//
// MIX holds batch x length samples, NOISE (optional) n_noise x batch x
// padded_length values; without it the noise comes from the library's own
// stream (ou_randn) at --seed (default 0).  Build line: INTEGRATION.md.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ouhip.h"

static int die(const char* what, const char* why)
{
    std::fprintf(stderr, "enhance_host: %s: %s\n", what, why);
    return 1;
}

static bool read_f32(const char* path, std::vector<float>& v, size_t n)
{
    v.resize(n);
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    const size_t got = std::fread(v.data(), sizeof(float), n, f);
    const bool more = std::fgetc(f) != EOF;
    std::fclose(f);
    return got == n && !more;
}

#define HIP_OK(e)                                                      \
    do {                                                               \
        hipError_t e_ = (e);                                           \
        if (e_ != hipSuccess) return die(#e, hipGetErrorString(e_));   \
    } while (0)

int main(int argc, char** argv)
{
    if (argc < 4) return die("usage", "enhance_host BUNDLE.oub MIX.f32 OUT.f32 [NOISE.f32 | --seed N]");
    const char* noise_path = nullptr;
    uint64_t seed = 0;
    if (argc >= 6 && !std::strcmp(argv[4], "--seed")) seed = std::strtoull(argv[5], nullptr, 10);
    else if (argc >= 5) noise_path = argv[4];

    ou_model* m = nullptr;
    if (ou_bundle_load(argv[1], 1, &m) != 0) return die("ou_bundle_load", ou_last_error());
    ou_bundle_meta info;
    if (ou_model_info(m, &info) != 0) return die("ou_model_info", ou_last_error());
    const size_t n_mix = (size_t)info.mix.batch * info.mix.length;
    const size_t n_noise = (size_t)info.noise.count * info.noise.batch * info.noise.length;
    std::fprintf(stderr, "enhance_host: batch %d, %d samples, %d noise draws of %d, %s\n", info.mix.batch,
                 info.mix.length, info.noise.count, info.noise.length, info.json);

    std::vector<float> mix, noise, out(n_mix);
    if (!read_f32(argv[2], mix, n_mix)) return die(argv[2], "expected batch x length float32 samples");
    if (noise_path && !read_f32(noise_path, noise, n_noise))
        return die(noise_path, "expected n_noise x batch x padded_length float32 values");

    hipStream_t stream = nullptr;
    float *d_mix = nullptr, *d_noise = nullptr, *d_out = nullptr;
    HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    HIP_OK(hipMalloc(&d_mix, n_mix * sizeof(float)));
    HIP_OK(hipMalloc(&d_out, n_mix * sizeof(float)));
    HIP_OK(hipMemcpyAsync(d_mix, mix.data(), n_mix * sizeof(float), hipMemcpyHostToDevice, stream));
    int rc;
    if (noise_path) {
        HIP_OK(hipMalloc(&d_noise, n_noise * sizeof(float)));
        HIP_OK(hipMemcpyAsync(d_noise, noise.data(), n_noise * sizeof(float), hipMemcpyHostToDevice, stream));
        rc = ou_model_enhance_noise(m, d_mix, d_noise, d_out, stream);
    } else {
        rc = ou_model_enhance(m, d_mix, d_out, seed, 0, stream);
    }
    if (rc != 0) return die("enhance", ou_last_error());
    rc = ou_model_status(m);   // waits for the stream
    if (rc != 0) return die(rc == 2 ? "range error (use a bundle exported with f32 operands)" : "status", ou_last_error());
    HIP_OK(hipMemcpy(out.data(), d_out, n_mix * sizeof(float), hipMemcpyDeviceToHost));

    FILE* f = std::fopen(argv[3], "wb");
    if (!f || std::fwrite(out.data(), sizeof(float), n_mix, f) != n_mix || std::fclose(f) != 0)
        return die(argv[3], "cannot write the output");
    ou_model_destroy(m);
    (void)hipFree(d_mix), (void)hipFree(d_noise), (void)hipFree(d_out);
    (void)hipStreamDestroy(stream);
    return 0;
}
