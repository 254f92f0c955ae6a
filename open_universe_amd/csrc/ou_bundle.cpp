// ou_bundle.cpp -- host layer of the exported enhance bundles (include/ouhip.h:
// the file layout, ou_bundle_open / _info / _region / _op / _materialize).
//
// Plain C++17: no HIP include and no HIP call, so the parser also builds as a
// stand-alone host program (tests/emu/bundle_parse.cpp, under a sanitizer).
// The header, the tables, the descriptors and the JSON are copied out of the
// file into exactly sized heap buffers and validated once, at open; only the
// regions' saved bytes stay in the mapping.  Nothing here trusts the file: a
// bundle that opens can be materialised at any set of region bases without a
// read or a write outside its descriptors.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ouhip.h"

// The library's error buffer (ou_common.h, which includes the HIP runtime):
// the same inline definitions, so that the linker folds them into the one
// thread-local buffer ou_last_error returns.
namespace ouhip_detail {
inline char* err_buf()
{
    static thread_local char buf[512] = {0};
    return buf;
}
}  // namespace ouhip_detail

inline int ou_fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(ouhip_detail::err_buf(), 512, fmt, ap);
    va_end(ap);
    return code;
}

#ifdef OU_BUNDLE_STANDALONE   // built without the rest of the library
extern "C" const char* ou_last_error(void) { return ouhip_detail::err_buf(); }
#endif

namespace {

constexpr uint32_t kFormat = 1;
constexpr size_t kHeader = 128, kRegionEnt = 32, kOpEnt = 64, kRelocEnt = 24, kIoEnt = 32;
constexpr int kMaxSide = 8, kMaxEvents = 4096;   // ou_program.hip's lane and event limits

struct Region {
    uint32_t kind;
    uint64_t bytes, off;
};
struct Op {
    uint32_t kind, desc_bytes;
    uint32_t first_reloc, n_relocs;
    std::vector<unsigned char> desc;
    char label[40];
};
struct Reloc {
    uint32_t op, desc_off, region;
    uint64_t region_off;
};

uint32_t rd32(const unsigned char* p)
{
    uint32_t v;
    std::memcpy(&v, p, 4);
    return v;
}
uint64_t rd64(const unsigned char* p)
{
    uint64_t v;
    std::memcpy(&v, p, 8);
    return v;
}

// FNV-1a, 64 bit: every step is a bijection of the state, so a change of any
// single byte changes the sum
constexpr uint64_t kFnvBasis = 0xcbf29ce484222325ull;
uint64_t fnv1a(uint64_t h, const unsigned char* p, uint64_t n)
{
    for (uint64_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}

size_t desc_size(uint32_t op)
{
    switch (op) {
    case OU_OP_CONV: return sizeof(ou_conv_desc);
    case OU_OP_GRU: return sizeof(ou_gru_desc);
    case OU_OP_EMBED: return sizeof(ou_embed_desc);
    case OU_OP_HEAD: return sizeof(ou_head_desc);
    case OU_OP_NORMALIZE: return sizeof(ou_norm_args);
    case OU_OP_INV_RMS: return sizeof(ou_rms_args);
    case OU_OP_RMS: return sizeof(ou_rms_args);
    case OU_OP_POWER: return sizeof(ou_power_args);
    case OU_OP_PAD: return sizeof(ou_pad_args);
    case OU_OP_SCALE: return sizeof(ou_scale_args);
    case OU_OP_FINISH: return sizeof(ou_finish_args);
    case OU_OP_SNAKE: return sizeof(ou_snake_desc);
    case OU_OP_MEMSET: return sizeof(ou_memset_desc);
    case OU_OP_ENSEMBLE: return sizeof(ou_ensemble_args);
    case OU_OP_BLOCK: return sizeof(ou_block_desc);
    case OU_OP_LANE: case OU_OP_SIGNAL: case OU_OP_WAIT: return sizeof(ou_sync_args);
    }
    return 0;
}

bool is_sync(uint32_t k) { return k == OU_OP_LANE || k == OU_OP_SIGNAL || k == OU_OP_WAIT; }

}  // namespace

struct ou_bundle {
    void* map = nullptr;
    size_t map_bytes = 0;
    std::vector<Region> regions;
    std::vector<Op> ops;
    std::vector<Reloc> relocs;
    std::string json;
    ou_bundle_meta meta{};
    ~ou_bundle()
    {
        if (map) munmap(map, map_bytes);
    }
};

namespace {

// The rules ou_program_validate applies to a program's lanes (ou_program.hip:
// validate_lanes and check_side_cycles), on the bundle's op list: ids in
// range, a side lane starts with a WAIT, an event is signalled before it is
// waited on, the list ends on lane 0 after joining every side lane that ran
// ops, and no side lane waits on itself through other side lanes.
int check_lanes(const std::vector<Op>& ops)
{
    int lane = 0, nl = 1;
    std::vector<int> seen(1, 1), last_sig(1, -1), ops_in(1, 0), recorded, ev_lane;
    auto id_of = [](const Op& o) { return (int)rd32(o.desc.data()); };
    for (const auto& o : ops) {
        if (!is_sync(o.kind)) {
            ops_in[lane]++;
            continue;
        }
        const int v = id_of(o);
        if (v < 0 || v >= (o.kind == OU_OP_LANE ? kMaxSide + 1 : kMaxEvents))
            return ou_fail(-1, "bundle: sync id %d out of range", v);
        if (o.kind == OU_OP_LANE) {
            if (v >= nl) {
                nl = v + 1;
                seen.resize(nl, 0), last_sig.resize(nl, -1), ops_in.resize(nl, 0);
            }
            lane = v;
            continue;
        }
        if ((int)recorded.size() <= v) recorded.resize(v + 1, 0), ev_lane.resize(v + 1, -1);
        if (o.kind == OU_OP_SIGNAL) {
            if (lane > 0 && !seen[lane]) return ou_fail(-1, "bundle: lane %d signals before it waited", lane);
            recorded[v] = 1;
            ev_lane[v] = lane;
            last_sig[lane] = v;
        } else {
            if (!recorded[v]) return ou_fail(-1, "bundle: wait on event %d before it is signalled", v);
            seen[lane] = 1;
        }
    }
    if (lane != 0) return ou_fail(-1, "bundle: the program must end on lane 0");
    std::vector<int> done(nl, 0);
    bool edge[kMaxSide + 1][kMaxSide + 1] = {};
    std::vector<int> sig_lane(ev_lane.size(), -1);
    int cur = 0;
    for (const auto& o : ops) {
        if (!is_sync(o.kind)) continue;
        const int v = id_of(o);
        if (o.kind == OU_OP_LANE) cur = v;
        else if (o.kind == OU_OP_SIGNAL) sig_lane[v] = cur;
        else {
            if (cur == 0 && ev_lane[v] > 0 && last_sig[ev_lane[v]] == v) done[ev_lane[v]] = 1;
            if (sig_lane[v] > 0 && cur > 0 && sig_lane[v] != cur) edge[cur][sig_lane[v]] = true;
        }
    }
    for (int l = 1; l < nl; ++l) {
        if (!ops_in[l]) continue;
        if (last_sig[l] < 0) return ou_fail(-1, "bundle: lane %d never signals lane 0", l);
        if (!done[l]) return ou_fail(-1, "bundle: lane 0 never joins lane %d", l);
    }
    for (int k = 1; k <= kMaxSide; ++k)
        for (int i = 1; i <= kMaxSide; ++i)
            for (int j = 1; j <= kMaxSide; ++j)
                if (edge[i][k] && edge[k][j]) edge[i][j] = true;
    for (int i = 1; i <= kMaxSide; ++i)
        if (edge[i][i]) return ou_fail(-1, "bundle: side lane %d waits on itself through other side lanes", i);
    return 0;
}

// [off, off + n) inside a file of `size` bytes, on a 64-byte boundary
bool section_ok(uint64_t off, uint64_t n, uint64_t size)
{
    return off % 64 == 0 && off >= kHeader && off <= size && n <= size - off;
}

int check_io(const ou_bundle_io& io, uint64_t need, const std::vector<Region>& regions, const char* what)
{
    if (io.region < 0 || (size_t)io.region >= regions.size()) return ou_fail(-1, "bundle: %s: no region %d", what, io.region);
    const uint64_t bytes = regions[io.region].bytes;
    if (io.offset < 0 || io.offset % 4 || (uint64_t)io.offset > bytes || need > bytes - (uint64_t)io.offset)
        return ou_fail(-1, "bundle: %s buffer leaves region %d", what, io.region);
    return 0;
}

int parse(ou_bundle* b, const unsigned char* f, uint64_t size)
{
    if (size < kHeader) return ou_fail(-1, "bundle: file of %llu bytes has no header", (unsigned long long)size);
    if (std::memcmp(f, "OUHB", 4) != 0) return ou_fail(-1, "bundle: missing OUHB marker");
    if (rd32(f + 4) != kFormat) return ou_fail(-2, "bundle: format version %u, expected %u", rd32(f + 4), kFormat);
    if (rd32(f + 8) != (uint32_t)OUHIP_ABI_VERSION)
        return ou_fail(-2, "bundle: written for ABI version %u, this library is %d", rd32(f + 8), OUHIP_ABI_VERSION);
    const uint64_t n_regions = rd32(f + 12), n_ops = rd32(f + 16), n_relocs = rd32(f + 20), n_json = rd32(f + 24);
    if (rd32(f + 28) != 0) return ou_fail(-1, "bundle: reserved header word set");
    for (size_t i = 112; i < kHeader; ++i)
        if (f[i]) return ou_fail(-1, "bundle: reserved header bytes set");
    std::memcpy(b->meta.arch, f + 32, 16);
    if (b->meta.arch[15] != 0) return ou_fail(-1, "bundle: arch string is not terminated");
    const uint64_t r_off = rd64(f + 48), o_off = rd64(f + 56), l_off = rd64(f + 64), io_off = rd64(f + 72),
                   j_off = rd64(f + 80);
    if (rd64(f + 88) != size)
        return ou_fail(-1, "bundle: header says %llu bytes, the file has %llu", (unsigned long long)rd64(f + 88),
                       (unsigned long long)size);
    if (n_regions < 1 || n_ops < 1) return ou_fail(-1, "bundle: no regions or no ops");
    // everything but the regions' saved bytes lies in [128, meta) and is covered by the checksum
    const uint64_t meta = rd64(f + 104);
    if (meta % 64 || meta < kHeader || meta > size) return ou_fail(-1, "bundle: tables end outside the file");
    if (!section_ok(r_off, n_regions * kRegionEnt, meta)) return ou_fail(-1, "bundle: region table outside the file");
    if (!section_ok(o_off, n_ops * kOpEnt, meta)) return ou_fail(-1, "bundle: op table outside the file");
    if (!section_ok(l_off, n_relocs * kRelocEnt, meta)) return ou_fail(-1, "bundle: relocation table outside the file");
    if (!section_ok(io_off, 4 * kIoEnt, meta)) return ou_fail(-1, "bundle: I/O table outside the file");
    if (!section_ok(j_off, n_json, meta)) return ou_fail(-1, "bundle: JSON outside the file");
    if (rd64(f + 96) != fnv1a(fnv1a(kFnvBasis, f, 96), f + kHeader, meta - kHeader))
        return ou_fail(-1, "bundle: header and tables do not match their checksum");

    b->regions.resize(n_regions);
    uint64_t total = 0;
    for (uint64_t i = 0; i < n_regions; ++i) {
        const unsigned char* e = f + r_off + i * kRegionEnt;
        Region& r = b->regions[i];
        r.kind = rd32(e), r.bytes = rd64(e + 8), r.off = rd64(e + 16);
        if (r.kind > 2 || (r.kind == 0) != (i == 0) || rd32(e + 4) != 0 || rd64(e + 24) != 0)
            return ou_fail(-1, "bundle: region %llu: bad kind %u", (unsigned long long)i, r.kind);
        if (r.bytes == 0 || r.bytes > (1ull << 40)) return ou_fail(-1, "bundle: region %llu: bad size", (unsigned long long)i);
        if (r.kind == 1 ? (r.off < meta || !section_ok(r.off, r.bytes, size)) : r.off != 0)
            return ou_fail(-1, "bundle: region %llu: saved bytes outside the file", (unsigned long long)i);
        total += (r.bytes + 255) / 256 * 256;
    }
    b->meta.region_bytes = (int64_t)total;

    b->ops.resize(n_ops);
    uint64_t next_reloc = 0;
    for (uint64_t i = 0; i < n_ops; ++i) {
        const unsigned char* e = f + o_off + i * kOpEnt;
        Op& o = b->ops[i];
        o.kind = rd32(e), o.desc_bytes = rd32(e + 4);
        const uint64_t d_off = rd64(e + 8);
        o.first_reloc = rd32(e + 16), o.n_relocs = rd32(e + 20);
        std::memcpy(o.label, e + 24, 40);
        if (o.label[39] != 0) return ou_fail(-1, "bundle: op %llu: label is not terminated", (unsigned long long)i);
        const size_t want = desc_size(o.kind);
        if (want == 0) return ou_fail(-1, "bundle: op %llu: unknown kind %u", (unsigned long long)i, o.kind);
        if (o.desc_bytes != want)
            return ou_fail(-1, "bundle: op %llu (kind %u): descriptor of %u bytes, expected %zu", (unsigned long long)i,
                           o.kind, o.desc_bytes, want);
        if (d_off % 8 || d_off < kHeader || d_off > meta || o.desc_bytes > meta - d_off)
            return ou_fail(-1, "bundle: op %llu: descriptor outside the file", (unsigned long long)i);
        if (o.first_reloc != next_reloc || o.n_relocs > n_relocs - next_reloc)
            return ou_fail(-1, "bundle: op %llu: relocation range out of step", (unsigned long long)i);
        next_reloc += o.n_relocs;
        o.desc.assign(f + d_off, f + d_off + o.desc_bytes);
    }
    if (next_reloc != n_relocs) return ou_fail(-1, "bundle: %llu relocations belong to no op", (unsigned long long)(n_relocs - next_reloc));

    b->relocs.resize(n_relocs);
    for (uint64_t i = 0; i < n_relocs; ++i) {
        const unsigned char* e = f + l_off + i * kRelocEnt;
        Reloc& r = b->relocs[i];
        r.op = rd32(e), r.desc_off = rd32(e + 4), r.region = rd32(e + 8), r.region_off = rd64(e + 16);
        if (rd32(e + 12) != 0) return ou_fail(-1, "bundle: relocation %llu: reserved word set", (unsigned long long)i);
        if (r.op >= n_ops || i < b->ops[r.op].first_reloc || i - b->ops[r.op].first_reloc >= b->ops[r.op].n_relocs)
            return ou_fail(-1, "bundle: relocation %llu is not in its op's range", (unsigned long long)i);
        const Op& o = b->ops[r.op];
        if (r.desc_off % 8 || r.desc_off > o.desc_bytes || o.desc_bytes - r.desc_off < 8)
            return ou_fail(-1, "bundle: relocation %llu leaves the descriptor of op %u", (unsigned long long)i, r.op);
        if (i > o.first_reloc && b->relocs[i - 1].desc_off >= r.desc_off)
            return ou_fail(-1, "bundle: relocation %llu: fields of op %u out of order", (unsigned long long)i, r.op);
        if (r.region >= n_regions || r.region_off >= b->regions[r.region].bytes)
            return ou_fail(-1, "bundle: relocation %llu (op %u) leaves region %u", (unsigned long long)i, r.op, r.region);
        if (rd64(o.desc.data() + r.desc_off) != 0)
            return ou_fail(-1, "bundle: relocation %llu: the stored field of op %u is not zero", (unsigned long long)i, r.op);
    }

    ou_bundle_io* ios[4] = {&b->meta.mix, &b->meta.noise, &b->meta.out, &b->meta.status};
    for (int k = 0; k < 4; ++k) {
        const unsigned char* e = f + io_off + k * kIoEnt;
        ou_bundle_io& io = *ios[k];
        io.region = (int32_t)rd32(e), io.count = (int32_t)rd32(e + 4), io.offset = (int64_t)rd64(e + 8);
        io.batch = (int32_t)rd32(e + 16), io.length = (int32_t)rd32(e + 20);
        if (rd64(e + 24) != 0) return ou_fail(-1, "bundle: I/O entry %d: reserved word set", k);
        if (io.count < 0 || io.batch < 0 || io.length < 0) return ou_fail(-1, "bundle: I/O entry %d: negative shape", k);
    }
    const ou_bundle_meta& m = b->meta;
    if (m.mix.batch < 1 || m.mix.length < 1 || m.out.batch != m.mix.batch || m.out.length != m.mix.length
        || m.noise.batch != m.mix.batch || m.noise.length <= m.mix.length || m.noise.count < 1
        || m.mix.count != 0 || m.out.count != 0 || m.status.count < 4 || m.status.batch != 0 || m.status.length != 0)
        return ou_fail(-1, "bundle: inconsistent I/O shapes");
    int rc;
    if ((rc = check_io(m.mix, 4ull * m.mix.batch * m.mix.length, b->regions, "mix"))) return rc;
    if ((rc = check_io(m.noise, 4ull * m.noise.count * m.noise.batch * m.noise.length, b->regions, "noise"))) return rc;
    if ((rc = check_io(m.out, 4ull * m.out.batch * m.out.length, b->regions, "out"))) return rc;
    if ((rc = check_io(m.status, 4ull * m.status.count, b->regions, "status"))) return rc;
    if (b->regions[m.status.region].kind == 1) return ou_fail(-1, "bundle: the status words must start zeroed");

    b->json.assign((const char*)f + j_off, n_json);
    if (b->json.find('\0') != std::string::npos) return ou_fail(-1, "bundle: NUL inside the JSON");
    b->meta.n_regions = (int32_t)n_regions;
    b->meta.n_ops = (int32_t)n_ops;
    b->meta.json = b->json.c_str();
    b->meta.json_bytes = (int64_t)n_json;
    return check_lanes(b->ops);
}

}  // namespace

extern "C" {

int ou_bundle_open(const char* path, ou_bundle** out)
{
    if (!path || !out) return ou_fail(-1, "bundle_open: null");
    *out = nullptr;
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return ou_fail(-3, "bundle_open: cannot open %s", path);
    struct stat st;
    if (fstat(fd, &st) != 0 || st.st_size <= 0) {
        close(fd);
        return ou_fail(-3, "bundle_open: %s is empty or unreadable", path);
    }
    ou_bundle* b = new ou_bundle();
    b->map_bytes = (size_t)st.st_size;
    b->map = mmap(nullptr, b->map_bytes, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (b->map == MAP_FAILED) {
        b->map = nullptr;
        delete b;
        return ou_fail(-3, "bundle_open: cannot map %s", path);
    }
    const int rc = parse(b, (const unsigned char*)b->map, (uint64_t)b->map_bytes);
    if (rc) {
        delete b;
        return rc;
    }
    *out = b;
    return 0;
}

void ou_bundle_close(ou_bundle* b) { delete b; }

int ou_bundle_info(const ou_bundle* b, ou_bundle_meta* meta)
{
    if (!b || !meta) return ou_fail(-1, "bundle_info: null");
    *meta = b->meta;
    return 0;
}

int ou_bundle_region(const ou_bundle* b, int i, int32_t* kind, int64_t* bytes, const void** data)
{
    if (!b) return ou_fail(-1, "bundle_region: null");
    if (i < 0 || (size_t)i >= b->regions.size()) return ou_fail(-1, "bundle_region: no region %d", i);
    const Region& r = b->regions[i];
    if (kind) *kind = (int32_t)r.kind;
    if (bytes) *bytes = (int64_t)r.bytes;
    if (data) *data = r.kind == 1 ? (const unsigned char*)b->map + r.off : nullptr;
    return 0;
}

int ou_bundle_op(const ou_bundle* b, int i, int32_t* kind, int64_t* desc_bytes, const char** label)
{
    if (!b) return ou_fail(-1, "bundle_op: null");
    if (i < 0 || (size_t)i >= b->ops.size()) return ou_fail(-1, "bundle_op: no op %d", i);
    const Op& o = b->ops[i];
    if (kind) *kind = (int32_t)o.kind;
    if (desc_bytes) *desc_bytes = (int64_t)o.desc_bytes;
    if (label) *label = o.label;
    return 0;
}

int ou_bundle_materialize(const ou_bundle* b, const uint64_t* region_bases, int op, void* desc_out)
{
    if (!b || !region_bases || !desc_out) return ou_fail(-1, "bundle_materialize: null");
    if (op < 0 || (size_t)op >= b->ops.size()) return ou_fail(-1, "bundle_materialize: no op %d", op);
    const Op& o = b->ops[op];
    std::memcpy(desc_out, o.desc.data(), o.desc.size());
    for (uint32_t k = 0; k < o.n_relocs; ++k) {
        const Reloc& r = b->relocs[o.first_reloc + k];   // inside the descriptor and the region: checked at open
        const uint64_t p = region_bases[r.region] + r.region_off;
        std::memcpy((unsigned char*)desc_out + r.desc_off, &p, 8);
    }
    return 0;
}

}  // extern "C"
