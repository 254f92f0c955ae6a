// stream_host.cpp -- a streaming enhance from a C++ host, without Python: load
// an exported bundle (python -m open_universe_amd.bin.export_bundle), push a
// raw little-endian float32 signal through a session chunk by chunk as a live
// source would deliver it, and write the samples each push makes final.
//
//   stream_host BUNDLE.oub IN.f32 OUT.f32 CHUNK OVERLAP [--seed N]
//
// CHUNK is the number of samples per push (any positive number: the result
// does not depend on it), OVERLAP the crossfade in samples, at most half the
// bundle's window.  The noise is the library's own stream (ou_randn) at --seed
// (default 0).  Build line: INTEGRATION.md.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ouhip.h"

static int die(const char* what, const char* why)
{
    std::fprintf(stderr, "stream_host: %s: %s\n", what, why);
    return 1;
}

#define HIP_OK(e)                                                      \
    do {                                                               \
        hipError_t e_ = (e);                                           \
        if (e_ != hipSuccess) return die(#e, hipGetErrorString(e_));   \
    } while (0)

int main(int argc, char** argv)
{
    if (argc < 6) return die("usage", "stream_host BUNDLE.oub IN.f32 OUT.f32 CHUNK OVERLAP [--seed N]");
    const long long chunk = std::atoll(argv[4]);
    const int overlap = std::atoi(argv[5]);
    uint64_t seed = 0;
    if (argc >= 8 && !std::strcmp(argv[6], "--seed")) seed = std::strtoull(argv[7], nullptr, 10);
    if (chunk < 1) return die(argv[4], "the chunk must be at least one sample");

    ou_model* m = nullptr;
    if (ou_bundle_load(argv[1], 1, &m) != 0) return die("ou_bundle_load", ou_last_error());
    ou_bundle_meta info;
    if (ou_model_info(m, &info) != 0) return die("ou_model_info", ou_last_error());
    ou_stream* s = nullptr;
    if (ou_model_stream_open(m, overlap, seed, 0, &s) != 0) return die("ou_model_stream_open", ou_last_error());
    std::fprintf(stderr, "stream_host: windows of %d samples, %d per replay, hop %d\n", info.mix.length,
                 info.mix.batch, info.mix.length - overlap);

    FILE* in = std::fopen(argv[2], "rb");
    FILE* out = std::fopen(argv[3], "wb");
    if (!in) return die(argv[2], "cannot read");
    if (!out) return die(argv[3], "cannot write");

    // a push emits whole hops of the groups it completes, close at most the ring: chunk + (B + 1) W bounds both
    const size_t cap_out = (size_t)chunk + ((size_t)info.mix.batch + 1) * info.mix.length;
    hipStream_t stream = nullptr;
    float *d_in = nullptr, *d_out = nullptr;
    HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    HIP_OK(hipMalloc(&d_in, (size_t)chunk * sizeof(float)));
    HIP_OK(hipMalloc(&d_out, cap_out * sizeof(float)));
    std::vector<float> h_in((size_t)chunk), h_out(cap_out);

    long long fed = 0, emitted = 0;
    // the samples a call made final: wait for them, check the replays, write them
    auto write_out = [&](int64_t got) -> int {
        if (got == 0) return 0;
        const int rc = ou_model_status(m);   // waits for the stream; an error ends the session
        if (rc != 0)
            return die(rc == 2 ? "range error (use a bundle exported with f32 operands)" : "status", ou_last_error());
        HIP_OK(hipMemcpy(h_out.data(), d_out, (size_t)got * sizeof(float), hipMemcpyDeviceToHost));
        if (std::fwrite(h_out.data(), sizeof(float), (size_t)got, out) != (size_t)got)
            return die(argv[3], "cannot write the output");
        emitted += got;
        return 0;
    };
    for (;;) {
        const size_t n = std::fread(h_in.data(), sizeof(float), (size_t)chunk, in);
        if (n > 0) {
            if ((size_t)ou_model_stream_bound(s, (int64_t)n, 0) > cap_out)
                return die("push", "output buffer too small");
            int64_t got = 0;
            HIP_OK(hipMemcpyAsync(d_in, h_in.data(), n * sizeof(float), hipMemcpyHostToDevice, stream));
            if (ou_model_stream_push(s, d_in, (int64_t)n, d_out, &got, stream) != 0)
                return die("ou_model_stream_push", ou_last_error());
            fed += (long long)n;
            if (write_out(got)) return 1;   // also orders the next copy into d_in behind this push
            if (got == 0) HIP_OK(hipStreamSynchronize(stream));
        }
        if (n < (size_t)chunk) break;
    }
    int64_t got = 0;
    const int rc = ou_model_stream_close(s, d_out, &got, stream);
    if (rc == OU_STREAM_SHORT) return die("the stream is shorter than one window", ou_last_error());
    if (rc != 0) return die("ou_model_stream_close", ou_last_error());
    if (write_out(got)) return 1;
    if (std::fclose(out) != 0) return die(argv[3], "cannot write the output");
    std::fclose(in);
    std::fprintf(stderr, "stream_host: %lld samples in, %lld out\n", fed, emitted);
    ou_model_stream_destroy(s);
    ou_model_destroy(m);
    (void)hipFree(d_in), (void)hipFree(d_out);
    (void)hipStreamDestroy(stream);
    return 0;
}
