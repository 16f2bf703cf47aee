// Engine files (include/s2m2_hip.h: s2m2_plan_save, s2m2_engine_*): one recorded forward written to disk together with the device memory its
// calls point to, and a loader / runner that needs nothing but this library and the HIP runtime.
//
// File layout (little-endian, every field naturally aligned; FORMAT_VERSION 1):
//   FileHeader                                  magic "S2M2ENG\0", format version, S2M2_ABI_VERSION, table sizes, s2m2_engine_info
//   FileRegion  x nregions                      kind, flags (zero / unused), bytes, stored bytes
//   FileCall    x ncalls                        entry point name, blob words, offset into the arena, pointer mask
//   FilePatch   x npatches                      (call, word) <- (region, offset); sorted by (call, word)
//   arena       x arena_words (u64)             the blobs; word 0 of every blob and every pointer word are 0 in the file
//   data                                        the stored bytes of the regions, in region order
// Every pointer word of a call is either null or covered by exactly one patch: no raw address is ever written or read back.
#include "common.h"
#include "plan.h"

#include <algorithm>
#include <atomic>
#include <memory>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

namespace {

constexpr char kMagic[8] = {'S', '2', 'M', '2', 'E', 'N', 'G', '\0'};
constexpr uint32_t kFormatVersion = 1;
constexpr int kNameBytes = 48;
constexpr uint32_t kFlagZero = 1, kFlagUnused = 2;               // stored as size only: all zero / no call points into it
constexpr size_t kRegionAlign = 4096;                            // >= the 512 bytes of torch's caching allocator
constexpr uint32_t kMaxRegions = 1u << 20, kMaxCalls = 1u << 20, kMaxPatches = 1u << 26;

struct FileHeader {
    char magic[8];
    uint32_t format, abi;
    uint32_t nregions, ncalls, npatches, info_bytes;
    uint64_t arena_words;
    uint64_t data_bytes;
    s2m2_engine_info info;
};
struct FileRegion { uint32_t kind, flags; uint64_t bytes, stored; };
struct FileCall { char name[kNameBytes]; uint32_t words, reserved; uint64_t off; uint64_t mask[s2m2::kPlanMaskWords]; };
struct FilePatch { uint32_t call, word, region, reserved; uint64_t offset; };

size_t image_elem_bytes(int image_dtype) { return image_dtype == S2M2_F32 ? 4 : image_dtype == S2M2_F16 ? 2 : 1; }
uint64_t out_bytes(const s2m2_engine_info& m) { return 3ull * (uint64_t)m.B * (uint64_t)m.out_h * (uint64_t)m.out_w * sizeof(float); }

bool mask_test(const uint64_t* mask, size_t w) { return w < 64 * (size_t)s2m2::kPlanMaskWords && ((mask[w / 64] >> (w % 64)) & 1ull) != 0; }

// the engine description shared by save and load: shapes consistent, result inside a region that is neither an input nor dropped
int check_info(const s2m2_engine_info& m, const std::vector<FileRegion>& regs, const char* who) {
    using s2m2::set_error;
    if (m.B <= 0 || m.H <= 0 || m.W <= 0 || m.H % 32 || m.W % 32 || m.B > 4096 || m.H > 65536 || m.W > 65536)
        return set_error("%s: bad engine shape B=%d H=%d W=%d", who, m.B, m.H, m.W);
    if ((m.dtype != S2M2_F32 && m.dtype != S2M2_F16) || (m.image_dtype < 0 || m.image_dtype > 2))
        return set_error("%s: bad dtypes (compute %d, image %d)", who, m.dtype, m.image_dtype);
    const int f = m.output_upsample ? 2 : 1;
    if (m.out_h != f * m.H || m.out_w != f * m.W) return set_error("%s: output %dx%d does not follow from %dx%d", who, m.out_h, m.out_w, m.H, m.W);
    if (m.out_region < 0 || m.out_region >= (int)regs.size() || regs[m.out_region].kind == S2M2_REGION_EXTERNAL ||
        (regs[m.out_region].flags & kFlagUnused) || m.out_offset < 0 || (uint64_t)m.out_offset > regs[m.out_region].bytes ||
        out_bytes(m) > regs[m.out_region].bytes - (uint64_t)m.out_offset)
        return set_error("%s: the result (region %d, offset %lld, %llu bytes) is not inside a region of the engine", who, m.out_region,
                         (long long)m.out_offset, (unsigned long long)out_bytes(m));
    int next = 0;
    const uint64_t img = (uint64_t)m.B * 3 * m.H * m.W * image_elem_bytes(m.image_dtype);
    for (const auto& r : regs) {
        if (r.kind != S2M2_REGION_EXTERNAL) continue;
        if (r.bytes != img) return set_error("%s: external %d holds %llu bytes, a (B,3,H,W) image %llu", who, next, (unsigned long long)r.bytes,
                                             (unsigned long long)img);
        ++next;
    }
    if (next != 2) return set_error("%s: %d external regions (the left and the right image: 2)", who, next);
    return 0;
}

struct File {
    FILE* f = nullptr;
    ~File() { if (f) fclose(f); }
};

}  // namespace

// ------------------------------------------------------------------------------------------------------------------------------------
extern "C" int s2m2_plan_save(const s2m2_plan* plan, const s2m2_engine_region* regions, int nregions, const s2m2_engine_info* meta,
                              const char* path) {
    using namespace s2m2;
    S2M2_REQUIRE(plan && plan->sealed && !plan->failed, "plan_save: the plan was not recorded to its end");
    S2M2_REQUIRE(plan->nslots == 0, "plan_save: the plan was recorded with %d external buffers (an engine declares its memory as regions)", plan->nslots);
    S2M2_REQUIRE(!plan->calls.empty(), "plan_save: the plan is empty");
    S2M2_REQUIRE(regions && nregions > 0 && (uint32_t)nregions <= kMaxRegions && meta && path, "plan_save: null pointer or bad region count %d", nregions);
    const int n = nregions;
    std::vector<FileRegion> regs(n);
    std::vector<int> order(n);
    for (int r = 0; r < n; ++r) {
        const auto& g = regions[r];
        S2M2_REQUIRE(g.base && g.bytes > 0 && g.kind >= S2M2_REGION_CONTENT && g.kind <= S2M2_REGION_EXTERNAL,
                     "plan_save: region %d (base %p, %llu bytes, kind %d) is not a device range of a known kind", r, g.base, g.bytes, g.kind);
        regs[r] = {(uint32_t)g.kind, 0u, g.bytes, 0ull};
        order[r] = r;
    }
    auto lo = [&](int r) { return (uint64_t)(uintptr_t)regions[r].base; };
    std::sort(order.begin(), order.end(), [&](int a, int b) { return lo(a) < lo(b); });
    for (int i = 1; i < n; ++i)
        S2M2_REQUIRE(lo(order[i]) >= lo(order[i - 1]) + regions[order[i - 1]].bytes, "plan_save: regions %d and %d overlap", order[i - 1], order[i]);
    auto find = [&](uint64_t v) -> int {                           // the region holding address v, -1: none
        int a = 0, b = n;                                          // first sorted index with base > v
        while (a < b) {
            const int m = (a + b) / 2;
            if (lo(order[m]) <= v) a = m + 1; else b = m;
        }
        if (a == 0) return -1;
        const int r = order[a - 1];
        return v - lo(r) < regions[r].bytes ? r : -1;
    };

    // calls: name -> table entry; every pointer word -> (region, offset) or null
    std::vector<FileCall> calls(plan->calls.size());
    std::vector<FilePatch> patches;
    std::vector<uint64_t> arena(plan->arena.begin(), plan->arena.end());
    std::vector<char> used(n, 0);
    for (size_t c = 0; c < plan->calls.size(); ++c) {
        const auto& call = plan->calls[c];
        const PlanEntry* e = plan_entry(call.name);
        S2M2_REQUIRE(e && e->tramp == call.tramp && (const void*)(uintptr_t)arena[call.off] == e->impl && (e->bytes + 7) / 8 == call.words &&
                     strlen(call.name) < (size_t)kNameBytes,
                     "plan_save: call %zu (%s) is not a registered recordable entry point (plan.h: S2M2_PLAN_ENTRY)", c, call.name);
        FileCall& fc = calls[c];
        memset(&fc, 0, sizeof(fc));
        strncpy(fc.name, call.name, kNameBytes - 1);
        fc.words = (uint32_t)call.words;
        fc.off = call.off;
        memcpy(fc.mask, call.mask.bits, sizeof(fc.mask));
        arena[call.off] = 0;                                       // the impl pointer: stored as the name
        for (size_t w = 1; w < call.words; ++w) {
            if (!call.mask.test(w)) continue;
            const uint64_t v = arena[call.off + w];
            if (v == 0) continue;
            const int r = find(v);
            S2M2_REQUIRE(r >= 0, "plan_save: call %zu (%s), pointer word %zu = %p falls in no region", c, call.name, w, (void*)(uintptr_t)v);
            S2M2_REQUIRE(regs[r].kind != S2M2_REGION_EXTERNAL || c == 0,
                         "plan_save: call %zu (%s), pointer word %zu points into external region %d (only the first call, the image prep, may)",
                         c, call.name, w, r);
            patches.push_back({(uint32_t)c, (uint32_t)w, (uint32_t)r, 0u, v - lo(r)});
            used[r] = 1;
            arena[call.off + w] = 0;
        }
    }
    S2M2_REQUIRE(strcmp(plan->calls[0].name, "s2m2_image_prep") == 0, "plan_save: the first call is %s, not s2m2_image_prep", plan->calls[0].name);
    S2M2_REQUIRE(meta->out_region >= 0 && meta->out_region < n, "plan_save: meta.out_region %d is not a region", meta->out_region);
    used[meta->out_region] = 1;
    for (int r = 0; r < n; ++r)
        if (!used[r] && regs[r].kind != S2M2_REGION_EXTERNAL) regs[r].flags |= kFlagUnused;
    if (check_info(*meta, regs, "plan_save")) return 1;

    // content: downloaded (the caller has synchronised), all-zero ranges stored as their size only
    std::vector<char> buf;
    auto chunk = [](uint64_t left) { return (size_t)std::min<uint64_t>(left, 64ull << 20); };
    for (int r = 0; r < n; ++r) {
        if (regs[r].kind != S2M2_REGION_CONTENT || (regs[r].flags & kFlagUnused)) continue;
        bool zero = true;
        for (uint64_t o = 0; o < regs[r].bytes && zero; o += chunk(regs[r].bytes - o)) {
            const size_t k = chunk(regs[r].bytes - o);
            buf.resize(k);
            S2M2_REQUIRE(hipMemcpy(buf.data(), (const char*)regions[r].base + o, k, hipMemcpyDeviceToHost) == hipSuccess,
                         "plan_save: cannot read region %d from the device", r);
            for (size_t i = 0; i < k && zero; ++i) zero = buf[i] == 0;
        }
        if (zero) regs[r].flags |= kFlagZero;
        else regs[r].stored = regs[r].bytes;
    }
    FileHeader h;
    memset(&h, 0, sizeof(h));
    memcpy(h.magic, kMagic, 8);
    h.format = kFormatVersion;
    h.abi = S2M2_ABI_VERSION;
    h.nregions = (uint32_t)n;
    h.ncalls = (uint32_t)calls.size();
    h.npatches = (uint32_t)patches.size();
    h.info_bytes = sizeof(s2m2_engine_info);
    h.arena_words = arena.size();
    for (const auto& r : regs) h.data_bytes += r.stored;
    h.info = *meta;

    const std::string tmp = std::string(path) + ".tmp";
    File out;
    out.f = fopen(tmp.c_str(), "wb");
    S2M2_REQUIRE(out.f, "plan_save: cannot open %s for writing", tmp.c_str());
    bool ok = fwrite(&h, sizeof(h), 1, out.f) == 1 && fwrite(regs.data(), sizeof(FileRegion), regs.size(), out.f) == regs.size() &&
              fwrite(calls.data(), sizeof(FileCall), calls.size(), out.f) == calls.size() &&
              (patches.empty() || fwrite(patches.data(), sizeof(FilePatch), patches.size(), out.f) == patches.size()) &&
              fwrite(arena.data(), 8, arena.size(), out.f) == arena.size();
    for (int r = 0; r < n && ok; ++r) {
        for (uint64_t o = 0; o < regs[r].stored && ok; o += chunk(regs[r].stored - o)) {
            const size_t k = chunk(regs[r].stored - o);
            buf.resize(k);
            ok = hipMemcpy(buf.data(), (const char*)regions[r].base + o, k, hipMemcpyDeviceToHost) == hipSuccess && fwrite(buf.data(), 1, k, out.f) == k;
        }
    }
    ok = fclose(out.f) == 0 && ok;
    out.f = nullptr;
    if (!ok || rename(tmp.c_str(), path) != 0) {
        remove(tmp.c_str());
        return set_error("plan_save: writing %s failed", path);
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------------------------
struct s2m2_engine {
    struct Call { const s2m2::PlanEntry* entry; size_t off, words; };
    struct ExtPatch { size_t word; int slot; uint64_t offset; };   // pointer words of call 0 into the images
    s2m2_engine_info info{};
    int device = 0;
    void* mem = nullptr;
    std::vector<uint64_t> arena;                                   // resolved blobs (call 0: image pointers patched per run)
    std::vector<Call> calls;
    std::vector<ExtPatch> ext;
    const float* out = nullptr;                                    // (3, B, 1, out_h, out_w) fp32 result of a run
    hipStream_t capture = nullptr;                                 // private stream the graph is captured on (never executes work)
    hipGraphExec_t exec = nullptr;
    long long runs = 0;
    std::atomic<int> busy{0};
};

namespace {

struct DeviceGuard {                                               // makes `dev` current for the scope, restores the caller's device
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

void release(s2m2_engine* e) {
    if (!e) return;
    if (!e->exec && !e->capture && !e->mem) {                      // failed on the host: nothing on a device to release
        delete e;
        return;
    }
    DeviceGuard g(e->device);
    if (e->exec) (void)hipGraphExecDestroy(e->exec);
    if (e->capture) (void)hipStreamDestroy(e->capture);
    if (e->mem) (void)hipFree(e->mem);
    delete e;
}

}  // namespace

extern "C" int s2m2_engine_load(const char* path, s2m2_engine** engine) {
    using namespace s2m2;
    S2M2_REQUIRE(path && engine, "engine_load: null pointer");
    *engine = nullptr;
    File in;
    in.f = fopen(path, "rb");
    S2M2_REQUIRE(in.f, "engine_load: cannot open %s", path);
    S2M2_REQUIRE(fseeko(in.f, 0, SEEK_END) == 0, "engine_load: %s: cannot seek", path);
    const uint64_t flen = (uint64_t)ftello(in.f);
    rewind(in.f);
    FileHeader h;
    S2M2_REQUIRE(flen >= sizeof(h) && fread(&h, sizeof(h), 1, in.f) == 1, "engine_load: %s: truncated header (%llu bytes, the header alone is %zu)",
                 path, (unsigned long long)flen, sizeof(h));
    S2M2_REQUIRE(memcmp(h.magic, kMagic, 8) == 0, "engine_load: %s is not an engine file (bad magic)", path);
    S2M2_REQUIRE(h.format == kFormatVersion, "engine_load: %s: file format version %u, this library reads %u", path, h.format, kFormatVersion);
    S2M2_REQUIRE(h.abi == (uint32_t)S2M2_ABI_VERSION, "engine_load: %s was written by ABI version %u, this library is %d: export it again",
                 path, h.abi, S2M2_ABI_VERSION);
    S2M2_REQUIRE(h.info_bytes == sizeof(s2m2_engine_info), "engine_load: %s: engine description of %u bytes, expected %zu", path, h.info_bytes,
                 sizeof(s2m2_engine_info));
    S2M2_REQUIRE(h.nregions >= 1 && h.nregions <= kMaxRegions && h.ncalls >= 1 && h.ncalls <= kMaxCalls && h.npatches <= kMaxPatches &&
                 h.arena_words <= (1ull << 32),
                 "engine_load: %s: implausible table sizes (%u regions, %u calls, %u patches, %llu arena words)", path, h.nregions, h.ncalls,
                 h.npatches, (unsigned long long)h.arena_words);
    const uint64_t tables = sizeof(h) + (uint64_t)h.nregions * sizeof(FileRegion) + (uint64_t)h.ncalls * sizeof(FileCall) +
                            (uint64_t)h.npatches * sizeof(FilePatch) + h.arena_words * 8;
    S2M2_REQUIRE(tables <= flen && h.data_bytes == flen - tables, "engine_load: %s: %llu bytes, the header describes %llu + %llu of data",
                 path, (unsigned long long)flen, (unsigned long long)tables, (unsigned long long)h.data_bytes);
    std::vector<FileRegion> regs(h.nregions);
    std::vector<FileCall> fcalls(h.ncalls);
    std::vector<FilePatch> patches(h.npatches);
    std::vector<uint64_t> arena(h.arena_words);
    S2M2_REQUIRE(fread(regs.data(), sizeof(FileRegion), regs.size(), in.f) == regs.size() &&
                 fread(fcalls.data(), sizeof(FileCall), fcalls.size(), in.f) == fcalls.size() &&
                 (patches.empty() || fread(patches.data(), sizeof(FilePatch), patches.size(), in.f) == patches.size()) &&
                 (arena.empty() || fread(arena.data(), 8, arena.size(), in.f) == arena.size()),
                 "engine_load: %s: read error", path);

    // regions: kinds, flags, stored sizes against the data section
    uint64_t data = 0;
    for (uint32_t r = 0; r < h.nregions; ++r) {
        const auto& g = regs[r];
        S2M2_REQUIRE(g.kind <= S2M2_REGION_EXTERNAL && g.bytes > 0 && g.bytes <= (1ull << 40) && (g.flags & ~(kFlagZero | kFlagUnused)) == 0,
                     "engine_load: %s: region %u is malformed (kind %u, flags %u, %llu bytes)", path, r, g.kind, g.flags, (unsigned long long)g.bytes);
        const bool stored = g.kind == S2M2_REGION_CONTENT && g.flags == 0;
        S2M2_REQUIRE(g.stored == (stored ? g.bytes : 0) && (g.kind == S2M2_REGION_CONTENT || (g.flags & kFlagZero) == 0) &&
                     (g.kind != S2M2_REGION_EXTERNAL || g.flags == 0),
                     "engine_load: %s: region %u stores %llu of %llu bytes (kind %u, flags %u)", path, r, (unsigned long long)g.stored,
                     (unsigned long long)g.bytes, g.kind, g.flags);
        data += g.stored;
    }
    S2M2_REQUIRE(data == h.data_bytes, "engine_load: %s: the regions store %llu bytes, the data section holds %llu", path, (unsigned long long)data,
                 (unsigned long long)h.data_bytes);
    if (check_info(h.info, regs, "engine_load")) return 1;

    // calls: known entry points with their blob sizes, blobs inside the arena in order, masks inside the blobs
    std::unique_ptr<s2m2_engine, void (*)(s2m2_engine*)> e(new s2m2_engine(), release);
    e->info = h.info;
    uint64_t next_off = 0;
    for (uint32_t c = 0; c < h.ncalls; ++c) {
        FileCall& fc = fcalls[c];
        S2M2_REQUIRE(memchr(fc.name, 0, kNameBytes) != nullptr, "engine_load: %s: call %u: entry point name not terminated", path, c);
        const PlanEntry* pe = plan_entry(fc.name);
        S2M2_REQUIRE(pe, "engine_load: %s: call %u names an unknown entry point '%s'", path, c, fc.name);
        S2M2_REQUIRE(fc.words == (pe->bytes + 7) / 8, "engine_load: %s: call %u (%s) has a blob of %u words, the entry point takes %zu", path, c,
                     fc.name, fc.words, (pe->bytes + 7) / 8);
        S2M2_REQUIRE(fc.off == next_off && fc.off + fc.words <= h.arena_words, "engine_load: %s: call %u (%s): blob at word %llu is not where the "
                     "previous one ends or runs past the arena", path, c, fc.name, (unsigned long long)fc.off);
        next_off += fc.words;
        S2M2_REQUIRE(!mask_test(fc.mask, 0) && arena[fc.off] == 0, "engine_load: %s: call %u (%s): word 0 is not the impl slot", path, c, fc.name);
        for (size_t w = fc.words; w < 64 * (size_t)kPlanMaskWords; ++w)
            S2M2_REQUIRE(!mask_test(fc.mask, w), "engine_load: %s: call %u (%s): pointer mask beyond the blob", path, c, fc.name);
        e->calls.push_back({pe, fc.off, fc.words});
    }
    S2M2_REQUIRE(next_off == h.arena_words, "engine_load: %s: %llu arena words, the calls use %llu", path, (unsigned long long)h.arena_words,
                 (unsigned long long)next_off);
    S2M2_REQUIRE(strcmp(fcalls[0].name, "s2m2_image_prep") == 0, "engine_load: %s: the first call is %s, not s2m2_image_prep", path, fcalls[0].name);

    // patches: sorted, on pointer words, inside live regions; images from call 0 only; every non-null pointer word patched
    std::vector<int> slot_of(h.nregions, -1);
    for (uint32_t r = 0, s = 0; r < h.nregions; ++r)
        if (regs[r].kind == S2M2_REGION_EXTERNAL) slot_of[r] = (int)s++;
    std::vector<char> patched(h.arena_words, 0);
    for (uint32_t i = 0; i < h.npatches; ++i) {
        const FilePatch& p = patches[i];
        S2M2_REQUIRE(p.call < h.ncalls && p.word >= 1 && p.word < fcalls[p.call].words && mask_test(fcalls[p.call].mask, p.word),
                     "engine_load: %s: patch %u targets call %u word %u, which is not a pointer word", path, i, p.call, p.word);
        S2M2_REQUIRE(i == 0 || p.call > patches[i - 1].call || (p.call == patches[i - 1].call && p.word > patches[i - 1].word),
                     "engine_load: %s: patch %u is out of order", path, i);
        S2M2_REQUIRE(p.region < h.nregions && !(regs[p.region].flags & kFlagUnused) && p.offset < regs[p.region].bytes,
                     "engine_load: %s: patch %u (call %u, %s, word %u): offset %llu is outside region %u", path, i, p.call, fcalls[p.call].name,
                     p.word, (unsigned long long)p.offset, p.region);
        S2M2_REQUIRE(slot_of[p.region] < 0 || p.call == 0, "engine_load: %s: call %u (%s) reads an input image (only the image prep may)", path,
                     p.call, fcalls[p.call].name);
        const uint64_t at = fcalls[p.call].off + p.word;
        S2M2_REQUIRE(arena[at] == 0, "engine_load: %s: patched word %u of call %u holds a raw value", path, p.word, p.call);
        patched[at] = 1;
    }
    for (uint32_t c = 0; c < h.ncalls; ++c)
        for (size_t w = 1; w < fcalls[c].words; ++w)
            S2M2_REQUIRE(!mask_test(fcalls[c].mask, w) || patched[fcalls[c].off + w] || arena[fcalls[c].off + w] == 0,
                         "engine_load: %s: call %u (%s), pointer word %zu holds a raw address", path, c, fcalls[c].name, w);

    // the device: a gfx950, then one allocation for every live region
    int dev = 0;
    S2M2_REQUIRE(hipGetDevice(&dev) == hipSuccess, "engine_load: no HIP device");
    hipDeviceProp_t prop;
    S2M2_REQUIRE(hipGetDeviceProperties(&prop, dev) == hipSuccess, "engine_load: cannot query device %d", dev);
    S2M2_REQUIRE(strncmp(prop.gcnArchName, "gfx950", 6) == 0, "engine_load: device %d is a %s; engines run on gfx950 (MI355X)", dev, prop.gcnArchName);
    e->device = dev;
    std::vector<uint64_t> at(h.nregions, ~0ull);
    uint64_t total = 0;
    for (uint32_t r = 0; r < h.nregions; ++r) {
        if (regs[r].kind == S2M2_REGION_EXTERNAL || (regs[r].flags & kFlagUnused)) continue;
        at[r] = total;
        total += (regs[r].bytes + kRegionAlign - 1) / kRegionAlign * kRegionAlign;
    }
    S2M2_REQUIRE(hipMalloc(&e->mem, total ? total : kRegionAlign) == hipSuccess, "engine_load: cannot allocate %llu bytes on device %d",
                 (unsigned long long)total, dev);
    S2M2_REQUIRE(hipMemset(e->mem, 0, total ? total : kRegionAlign) == hipSuccess, "engine_load: cannot clear the engine's memory");
    char* base = static_cast<char*>(e->mem);
    std::vector<char> buf;
    for (uint32_t r = 0; r < h.nregions; ++r) {
        for (uint64_t o = 0; o < regs[r].stored;) {
            const size_t k = (size_t)std::min<uint64_t>(regs[r].stored - o, 64ull << 20);
            buf.resize(k);
            S2M2_REQUIRE(fread(buf.data(), 1, k, in.f) == k, "engine_load: %s: read error in the data of region %u", path, r);
            S2M2_REQUIRE(hipMemcpy(base + at[r] + o, buf.data(), k, hipMemcpyHostToDevice) == hipSuccess, "engine_load: upload of region %u failed", r);
            o += k;
        }
    }
    for (const auto& c : e->calls) arena[c.off] = (uint64_t)(uintptr_t)c.entry->impl;
    for (const FilePatch& p : patches) {
        if (slot_of[p.region] >= 0) e->ext.push_back({(size_t)p.word, slot_of[p.region], p.offset});
        else arena[fcalls[p.call].off + p.word] = (uint64_t)(uintptr_t)(base + at[p.region] + p.offset);
    }
    e->arena.swap(arena);
    e->out = reinterpret_cast<const float*>(base + at[h.info.out_region] + h.info.out_offset);
    S2M2_REQUIRE(hipStreamCreateWithFlags(&e->capture, hipStreamNonBlocking) == hipSuccess, "engine_load: cannot create the capture stream");
    S2M2_REQUIRE(hipDeviceSynchronize() == hipSuccess, "engine_load: the upload failed");
    *engine = e.release();
    return 0;
}

extern "C" int s2m2_engine_meta(const s2m2_engine* engine, s2m2_engine_info* meta) {
    S2M2_REQUIRE(engine && meta, "engine_meta: null pointer");
    *meta = engine->info;
    return 0;
}

namespace {
int run_calls(const s2m2_engine* e, hipStream_t stream) {           // calls 1.. as recorded (their blobs are fully resolved)
    for (size_t c = 1; c < e->calls.size(); ++c)
        if (e->calls[c].entry->tramp(e->arena.data() + e->calls[c].off, stream) != 0) return 1;
    return 0;
}

int run_locked(s2m2_engine* e, const void* left, const void* right, float* disp, float* occ, float* conf, hipStream_t stream) {
    using namespace s2m2;
    // the image prep, eagerly, from the caller's images
    const auto& c0 = e->calls[0];
    std::vector<uint64_t> blob(e->arena.begin() + c0.off, e->arena.begin() + c0.off + c0.words);
    const void* img[2] = {left, right};
    for (const auto& x : e->ext) blob[x.word] = (uint64_t)(uintptr_t)img[x.slot] + x.offset;
    if (c0.entry->tramp(blob.data(), stream) != 0) return 1;
    const char* g = getenv("S2M2_GRAPH");
    const bool graph = !(g && strcmp(g, "0") == 0);
    if (!graph || e->runs == 0) {                                  // the first run is eager: lazy set-up (LDS reservations, zero page)
        if (run_calls(e, stream)) return 1;
    } else {
        if (!e->exec) {
            S2M2_REQUIRE(hipStreamBeginCapture(e->capture, hipStreamCaptureModeThreadLocal) == hipSuccess, "engine_run: cannot begin the capture");
            const int rc = run_calls(e, e->capture);
            hipGraph_t gr = nullptr;
            const hipError_t ec = hipStreamEndCapture(e->capture, &gr);
            if (rc != 0 || ec != hipSuccess || !gr) {
                if (gr) (void)hipGraphDestroy(gr);
                return rc ? 1 : set_error("engine_run: the capture failed: %s", hipGetErrorString(ec));
            }
            const hipError_t ei = hipGraphInstantiate(&e->exec, gr, nullptr, nullptr, 0);
            (void)hipGraphDestroy(gr);
            if (ei != hipSuccess) {
                e->exec = nullptr;
                return set_error("engine_run: cannot instantiate the graph: %s", hipGetErrorString(ei));
            }
        }
        S2M2_REQUIRE(hipGraphLaunch(e->exec, stream) == hipSuccess, "engine_run: graph launch failed");
    }
    ++e->runs;
    const size_t map = (size_t)e->info.B * e->info.out_h * e->info.out_w * sizeof(float);
    float* dst[3] = {disp, occ, conf};
    for (int k = 0; k < 3; ++k)
        S2M2_REQUIRE(hipMemcpyAsync(dst[k], reinterpret_cast<const char*>(e->out) + k * map, map, hipMemcpyDeviceToDevice, stream) == hipSuccess,
                     "engine_run: copying the result out failed");
    return 0;
}
}  // namespace

extern "C" int s2m2_engine_run(s2m2_engine* engine, const void* left, const void* right, float* disp, float* occ, float* conf, void* stream) {
    using namespace s2m2;
    S2M2_REQUIRE(engine && left && right && disp && occ && conf, "engine_run: null pointer");
    S2M2_REQUIRE(engine->busy.exchange(1) == 0, "engine_run: the engine is running on another thread (one run at a time per engine)");
    int rc;
    {
        DeviceGuard guard(engine->device);
        rc = guard.ok ? run_locked(engine, left, right, disp, occ, conf, static_cast<hipStream_t>(stream))
                      : set_error("engine_run: cannot make device %d current", engine->device);
    }
    engine->busy.store(0);
    return rc;
}

extern "C" int s2m2_engine_destroy(s2m2_engine* engine) {
    release(engine);
    return 0;
}
