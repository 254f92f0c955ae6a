// bundle_parse.cpp -- the bundle parser (csrc/ou_bundle.cpp, host only)
// against damaged files, as a stand-alone program for a sanitizer build:
//
//   bundle_parse <valid bundle> <scratch file>
//
// Every damaged file must be refused by ou_bundle_open (or, where it parses,
// by ou_bundle_materialize) with a message in ou_last_error; the sanitizer
// reports any read or write the parser makes outside its buffers on the way.
// Cases, from a fixed seed: every truncation at 64-byte strides, 2000
// single-byte corruptions of the header and tables (not of the regions' saved
// bytes), a relocation one byte past its region, a descriptor size off by 8,
// an ABI version off by one -- the last three with the checksum made right
// again, so that the check under test is the one that refuses them.
#include <fcntl.h>
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ouhip.h"

static int fails = 0;

static uint64_t fnv1a(uint64_t h, const unsigned char* p, uint64_t n)
{
    for (uint64_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}

template <class T>
static T rd(const std::vector<unsigned char>& f, size_t off)
{
    T v;
    std::memcpy(&v, f.data() + off, sizeof(T));
    return v;
}
template <class T>
static void wr(std::vector<unsigned char>& f, size_t off, T v)
{
    std::memcpy(f.data() + off, &v, sizeof(T));
}

static void resum(std::vector<unsigned char>& f)
{
    const uint64_t meta = rd<uint64_t>(f, 104);
    wr<uint64_t>(f, 96, fnv1a(fnv1a(0xcbf29ce484222325ull, f.data(), 96), f.data() + 128, meta - 128));
}

// the file must be refused, with a message (want: a piece of it, or null)
static void must_refuse(const char* path, const char* what, long long arg, const char* want = nullptr)
{
    ou_bundle* b = nullptr;
    int rc = ou_bundle_open(path, &b);
    if (rc == 0) {
        ou_bundle_meta m;
        ou_bundle_info(b, &m);
        std::vector<uint64_t> bases(m.n_regions, 1ull << 32);
        for (int i = 0; i < m.n_ops && rc == 0; ++i) {
            int64_t bytes = 0;
            ou_bundle_op(b, i, nullptr, &bytes, nullptr);
            std::vector<unsigned char> d((size_t)bytes);
            rc = ou_bundle_materialize(b, bases.data(), i, d.data());
        }
        ou_bundle_close(b);
    }
    const char* msg = ou_last_error();
    if (rc >= 0 || !msg || !msg[0] || (want && !std::strstr(msg, want))) {
        std::fprintf(stderr, "FAIL %s %lld: rc %d, message '%s'\n", what, arg, rc, msg ? msg : "");
        ++fails;
    }
}

static void write_at(int fd, const std::vector<unsigned char>& f, size_t off, size_t n)
{
    if (pwrite(fd, f.data() + off, n, (off_t)off) != (ssize_t)n) {
        std::perror("pwrite");
        std::exit(2);
    }
}

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    const char* scratch = argv[2];
    std::vector<unsigned char> good;
    {
        FILE* fp = std::fopen(argv[1], "rb");
        if (!fp) return 2;
        std::fseek(fp, 0, SEEK_END);
        good.resize((size_t)std::ftell(fp));
        std::fseek(fp, 0, SEEK_SET);
        if (std::fread(good.data(), 1, good.size(), fp) != good.size()) return 2;
        std::fclose(fp);
    }
    const int fd = open(scratch, O_RDWR | O_CREAT | O_TRUNC, 0600);
    if (fd < 0) return 2;
    write_at(fd, good, 0, good.size());

    // the untouched copy opens, and every op materialises
    {
        ou_bundle* b = nullptr;
        if (ou_bundle_open(scratch, &b) != 0) {
            std::fprintf(stderr, "FAIL: the valid bundle does not open: %s\n", ou_last_error());
            return 1;
        }
        ou_bundle_close(b);
    }
    const uint64_t meta = rd<uint64_t>(good, 104), o_off = rd<uint64_t>(good, 56), l_off = rd<uint64_t>(good, 64);
    const uint64_t r_off = rd<uint64_t>(good, 48);
    long long cases = 0;

    // single-byte corruptions of the header and tables
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto next = [&s]() {
        s ^= s << 13, s ^= s >> 7, s ^= s << 17;
        return s;
    };
    for (int k = 0; k < 2000; ++k, ++cases) {
        const size_t off = (size_t)(next() % meta);
        std::vector<unsigned char> one(1, (unsigned char)(good[off] ^ (1 + next() % 255)));
        if (pwrite(fd, one.data(), 1, (off_t)off) != 1) return 2;
        must_refuse(scratch, "corrupt byte", (long long)off);
        write_at(fd, good, off, 1);
    }
    // targeted damage, checksum restored
    {
        std::vector<unsigned char> f(good.begin(), good.begin() + (size_t)meta);
        const uint32_t region = rd<uint32_t>(f, l_off + 8);
        wr<uint64_t>(f, l_off + 16, rd<uint64_t>(f, r_off + 32 * region + 8));   // offset = the region's size
        resum(f);
        write_at(fd, f, 0, f.size());
        must_refuse(scratch, "relocation past its region", 0, "leaves region");
        f.assign(good.begin(), good.begin() + (size_t)meta);
        wr<uint32_t>(f, o_off + 4, rd<uint32_t>(f, o_off + 4) + 8);
        resum(f);
        write_at(fd, f, 0, f.size());
        must_refuse(scratch, "descriptor size", 0, "descriptor of");
        f.assign(good.begin(), good.begin() + (size_t)meta);
        wr<uint32_t>(f, 8, rd<uint32_t>(f, 8) + 1);
        resum(f);
        write_at(fd, f, 0, f.size());
        must_refuse(scratch, "ABI version", 0, "ABI version");
        write_at(fd, good, 0, (size_t)meta);
        cases += 3;
    }
    // truncations, from the end down
    for (long long size = (long long)((good.size() - 1) / 64 * 64); size >= 0; size -= 64, ++cases) {
        if (ftruncate(fd, (off_t)size) != 0) return 2;
        must_refuse(scratch, "truncation", size);
    }
    close(fd);
    if (fails) return 1;
    std::printf("ok: %lld damaged files refused\n", cases);
    return 0;
}
