// Model-specialised cascade kernels: hiprtc compiles wb_cascade_tile.h -- the SAME source the generic kernels are
// built from -- behind a generated prelude that makes the stage records of ONE model compile-time constants
// (wb_model_specialize).  Feature offsets become LDS instruction offsets, thresholds, leaf values and theta become
// literals, the scalar record loads and the moves in front of the selects disappear from phase A and from the
// wave-synchronous segments.  The generic kernels stay the cold path (and the only path for float32 tiles).
//
// Replaces nothing new of the reference: it is wb_cascade_launch's kernel (model.py:216-259, training.py:84-96)
// for a model that is scanned often enough to be worth ~2 s of compilation.  Compiled code objects are kept in
// the process and in a cache directory ($WB_JIT_CACHE, default ~/.cache/waldboost_amd), keyed by a hash of the
// generated source, the target and the hiprtc version.
#include <hip/hiprtc.h>
#include <stdlib.h>
#include <string.h>
#include <dirent.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>

#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "wb_common.h"

namespace {

const char kTileSrc[] =
#include "wb_cascade_tile.inc"
    ;

struct JitKernel {
    hipModule_t module = nullptr;
    hipFunction_t func = nullptr;
    int users = 0;                            // models holding the function (wb_jit_get / wb_jit_release)
    uint64_t released = 0;                    // when the last of them let go (a counter): the oldest idle module goes first
};

std::mutex g_mu;
std::map<uint64_t, JitKernel> g_loaded;      // per process: hash -> loaded module
uint64_t g_release_clock = 0;

uint64_t fnv1a(const void *p, size_t n, uint64_t h = 1469598103934665603ull) {
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < n; ++i) {
        h ^= b[i];
        h *= 1099511628211ull;
    }
    return h;
}

// the stage segments run_segments walks for a cascade of T stages (wb_cascade_tile.h: t_end = min(2 t, T, t + 64),
// from stage 8 on; the re-count at stage 16 splits nothing: 16 is on the chain)
// Only the segments that end by stage WB_JIT_BAKE_STAGES (default 384) are unrolled with their records as constants: the
// windows of a long soft cascade that get that far are a handful per tile, and a wave that walks them streams through its
// code once -- unrolled, stages 384..1023 would be hundreds of KB of instructions nobody executes twice; they run the
// generic segment loop of the same kernel (records through the scalar cache).
std::string segment_list(int T) {
    static const int cap = getenv("WB_JIT_BAKE_STAGES") ? atoi(getenv("WB_JIT_BAKE_STAGES")) : 384;
    std::string s;
    for (int t = 8; t < T;) {
        int e = 2 * t < T ? 2 * t : T;
        e = e < t + 64 ? e : t + 64;
        if (e > cap && t >= 16) break;
        s += " X(" + std::to_string(t) + "," + std::to_string(e) + ")";
        t = e;
    }
    return s;
}

std::string make_source(const int32_t *words, size_t n_words, int T, int D, int rpw, int waves, int C, int rows, int pitch, int eb = 1, int lds_stages = -1, int occ_min = 8) {
    std::string s;
    s.reserve(n_words * 12 + 1024);
    s += "#define WB_JIT_BAKED 1\n#define WB_JIT_STAGE_WORDS ";
    for (size_t i = 0; i < n_words; ++i) {
        if (i) s += ',';
        s += std::to_string(words[i]);
    }
    s += "\n#define WB_JIT_SEGMENTS(X)" + segment_list(T) + "\n";
    s += "#define WB_JIT_LDS_STAGES " + std::to_string(lds_stages < 0 ? T : lds_stages) + "\n";
    // (the occupancy floor can be overridden per build through WB_JIT_DEFS: diagnostics)
    s += "#define WB_JIT_RPW " + std::to_string(rpw) + "\n";
    s += "#define WB_JIT_WAVES " + std::to_string(waves) + "\n#ifndef WB_JIT_OCC_MIN\n#define WB_JIT_OCC_MIN " + std::to_string(occ_min) +
         "\n#endif\n#ifndef WB_JIT_ATTR_EXTRA\n#define WB_JIT_ATTR_EXTRA\n#endif\n";
    s += "#define WB_JIT_T " + std::to_string(T) + "\n#define WB_JIT_C " + std::to_string(C) + "\n#define WB_JIT_ROWS " +
         std::to_string(rows) + "\n#define WB_JIT_PITCH " + std::to_string(pitch) + "\n";
    s += "#include \"wb_cascade_tile.h\"\n";
    // (8 waves per SIMD, as the generic kernel reaches on its own with 41 registers: the byte tile admits 4 workgroups per CU)
    s += "extern \"C\" __global__ __launch_bounds__(" + std::to_string(waves * 64) +
         ") __attribute__((" + std::string(occ_min == 8 ? "amdgpu_num_sgpr(80), " : "") + "amdgpu_waves_per_eu(WB_JIT_OCC_MIN, 8) WB_JIT_ATTR_EXTRA)) void wb_casc_jit(CascArgs a, const int32_t *stages) {\n"
         "    cascade_tile_body<" + std::to_string(D) + ", " + std::to_string(rpw) + ", " + std::to_string(waves) +
         ", " + std::to_string(eb) + ", true>(a, stages);\n}\n";
    return s;
}

std::string cache_dir() {
    if (const char *e = getenv("WB_JIT_CACHE")) return *e ? std::string(e) : std::string();
    if (const char *h = getenv("HOME")) return std::string(h) + "/.cache/waldboost_amd";
    return std::string();
}

bool read_file(const std::string &path, std::vector<char> &out) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    out.resize(n > 0 ? (size_t)n : 0);
    const bool ok = n > 0 && fread(out.data(), 1, (size_t)n, f) == (size_t)n;
    fclose(f);
    return ok;
}

// The disk cache is bounded: before a new code object is written, the oldest ones (by modification time) go until at most
// WB_JIT_CACHE_MAX - 1 (default 256) are left -- a loop that changes its model every iteration (training with the uint8
// channel functions, threshold sweeps) otherwise leaves one file per model content behind, for ever.
void prune_cache(const std::string &dir) {
    const int cap = getenv("WB_JIT_CACHE_MAX") ? atoi(getenv("WB_JIT_CACHE_MAX")) : 256;
    DIR *d = opendir(dir.c_str());
    if (!d) return;
    std::vector<std::pair<time_t, std::string>> files;
    while (struct dirent *e = readdir(d)) {
        const std::string n = e->d_name;
        if (n.size() != 19 || n.compare(16, 3, ".co") != 0) continue;          // (only what this cache wrote: <16 hex digits>.co)
        struct stat st;
        if (stat((dir + "/" + n).c_str(), &st) == 0) files.emplace_back(st.st_mtime, n);
    }
    closedir(d);
    if ((int)files.size() < cap) return;
    std::sort(files.begin(), files.end());
    for (size_t i = 0; i + (size_t)(cap > 0 ? cap - 1 : 0) < files.size(); ++i) (void)unlink((dir + "/" + files[i].second).c_str());
}

// a cached file is only handed to the module loader if it looks like what compile() produces: an ELF image of plausible
// size, owned by this user (WB_JIT_CACHE may point at a shared directory)
bool plausible_code_object(const std::string &path, const std::vector<char> &code) {
    struct stat st;
    if (stat(path.c_str(), &st) != 0 || st.st_uid != geteuid() || (st.st_mode & (S_IWGRP | S_IWOTH))) return false;
    return code.size() > 64 && code[0] == 0x7f && code[1] == 'E' && code[2] == 'L' && code[3] == 'F';
}

void write_file_atomic(const std::string &dir, const std::string &path, const std::vector<char> &data) {
    if (dir.empty()) return;
    const size_t slash = dir.rfind('/');
    if (slash != std::string::npos && slash > 0) (void)mkdir(dir.substr(0, slash).c_str(), 0755);
    (void)mkdir(dir.c_str(), 0755);
    prune_cache(dir);
    const std::string tmp = path + "." + std::to_string((long)getpid()) + ".tmp";
    FILE *f = fopen(tmp.c_str(), "wb");
    if (!f) return;
    const bool ok = fwrite(data.data(), 1, data.size(), f) == data.size();
    fclose(f);
    if (!ok || rename(tmp.c_str(), path.c_str()) != 0) (void)unlink(tmp.c_str());
}

// source -> code object for `arch` (no HIP runtime call: works without a GPU)
int compile(const std::string &src, const char *arch, std::vector<char> &code, std::string &log) {
    hiprtcProgram prog;
    const char *hdr_src[] = {kTileSrc};
    const char *hdr_name[] = {"wb_cascade_tile.h"};
    hiprtcResult r = hiprtcCreateProgram(&prog, src.c_str(), "wb_casc_jit.hip", 1, hdr_src, hdr_name);
    if (r != HIPRTC_SUCCESS) {
        log = std::string("hiprtcCreateProgram: ") + hiprtcGetErrorString(r);
        return WB_ERR_HIP;
    }
    const std::string a = std::string("--offload-arch=") + arch;
    std::vector<std::string> extra;                          // diagnostic: WB_JIT_DEFS="-DWB_TAIL_PRIO=0 -D..." (A/B builds)
    if (const char *e = getenv("WB_JIT_DEFS")) {
        std::string cur;
        for (const char *c = e;; ++c) {
            if (*c == ' ' || *c == 0) {
                if (!cur.empty()) extra.push_back(cur);
                cur.clear();
                if (!*c) break;
            } else {
                cur += *c;
            }
        }
    }
    std::vector<const char *> opts = {a.c_str(), "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-pragma-once-outside-header", "-Wno-inline-asm"};
    for (const std::string &x : extra) opts.push_back(x.c_str());
    r = hiprtcCompileProgram(prog, (int)opts.size(), opts.data());
    size_t ls = 0;
    if (hiprtcGetProgramLogSize(prog, &ls) == HIPRTC_SUCCESS && ls > 1) {
        log.resize(ls);
        (void)hiprtcGetProgramLog(prog, &log[0]);
    }
    if (getenv("WB_JIT_VERBOSE") && !log.empty()) fprintf(stderr, "[wb_jit] %s\n", log.c_str());
    if (r != HIPRTC_SUCCESS) {
        const size_t at = log.find("error:");                     // (warnings first: show the first error)
        if (at != std::string::npos) log = log.substr(at > 120 ? at - 120 : 0);
        log = std::string("hiprtcCompileProgram: ") + hiprtcGetErrorString(r) + "\n" + log;
        (void)hiprtcDestroyProgram(&prog);
        return WB_ERR_HIP;
    }
    size_t cs = 0;
    r = hiprtcGetCodeSize(prog, &cs);
    if (r == HIPRTC_SUCCESS) {
        code.resize(cs);
        r = hiprtcGetCode(prog, code.data());
    }
    (void)hiprtcDestroyProgram(&prog);
    if (const char *d = getenv("WB_JIT_DUMP_DIR")) {            // diagnostic: the generated source and the code object
        const std::string base = std::string(d) + "/wb_casc_jit";
        if (FILE *f = fopen((base + ".hip").c_str(), "w")) { fwrite(src.data(), 1, src.size(), f); fclose(f); }
        if (FILE *f = fopen((base + ".co").c_str(), "wb")) { fwrite(code.data(), 1, code.size(), f); fclose(f); }
    }
    if (r != HIPRTC_SUCCESS || code.empty()) {
        log = std::string("hiprtcGetCode: ") + hiprtcGetErrorString(r);
        return WB_ERR_HIP;
    }
    return WB_OK;
}

// Bytes of scratch (private segment) per work-item the code object's kernel asks for, from its metadata note (msgpack:
// the key ".private_segment_fixed_size" followed by an unsigned integer); -1 when the note cannot be read.
int scratch_bytes(const std::vector<char> &code) {
    static const char key[] = ".private_segment_fixed_size";
    const size_t kl = sizeof(key) - 1;
    for (size_t i = 0; i + kl + 1 <= code.size(); ++i) {
        if (code[i] != key[0] || memcmp(code.data() + i, key, kl) != 0) continue;
        const unsigned char *v = reinterpret_cast<const unsigned char *>(code.data()) + i + kl;
        const size_t left = code.size() - i - kl;
        if (v[0] <= 0x7f) return v[0];
        if (v[0] == 0xcc && left >= 2) return v[1];
        if (v[0] == 0xcd && left >= 3) return (v[1] << 8) | v[2];
        if (v[0] == 0xce && left >= 5) return (int)(((uint32_t)v[1] << 24) | (v[2] << 16) | (v[3] << 8) | v[4]);
        return -1;
    }
    return -1;
}

// Scratch memory: every cascade kernel of the library keeps its state in registers and LDS, and a specialised build is
// expected to.  What used to send two lane addresses of a depth-3 or 1024-stage build to scratch is dealt with in the
// source (wb_cascade_tile.h: relane, WB_INLINE_LAMBDA).  wb_model_specialize accepts a build that asks for scratch anyway
// (its self-test decides); wb_jit_compile_check (the CPU suite) is strict: scratch fails the check.
int build_checked(const std::string &src, const char *arch, std::vector<char> &code, std::string &log) {
    const int rc = compile(src, arch, code, log);
    if (rc != WB_OK) return rc;
    const int sb = scratch_bytes(code);
    if (sb == 0) return WB_OK;
    code.clear();
    log = sb < 0 ? "the code object's metadata has no readable .private_segment_fixed_size"
                 : "the specialised kernel would spill registers to scratch memory (" + std::to_string(sb) + " bytes per lane)";
    return WB_ERR_UNSUPPORTED;
}

}  // namespace

namespace {
void evict_idle_modules();
}

// Build (or fetch) the specialised kernel for one stage table of `M`.  words: (T + G) records of SD dwords as uploaded.
int wb_jit_get(const int32_t *words, size_t n_words, int T, int D, int rpw, int waves, int C, int rows, int pitch, int eb, int lds_stages,
               void **func_out) {
    *func_out = nullptr;
    hipDeviceProp_t prop;
    int dev = 0;
    WB_HIP_CHECK(hipGetDevice(&dev));
    WB_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    const std::string src = make_source(words, n_words, T, D, rpw, waves, C, rows, pitch, eb, lds_stages);
    int rtc_major = 0, rtc_minor = 0;
    (void)hiprtcVersion(&rtc_major, &rtc_minor);
    uint64_t h = fnv1a(src.data(), src.size());
    h = fnv1a(kTileSrc, sizeof(kTileSrc), h);
    h = fnv1a(prop.gcnArchName, strlen(prop.gcnArchName), h);
    h = fnv1a(&rtc_major, sizeof(int), fnv1a(&rtc_minor, sizeof(int), h));
    h = fnv1a(&dev, sizeof(int), h);                         // (a module is loaded per device)
    if (const char *e = getenv("WB_JIT_DEFS")) h = fnv1a(e, strlen(e), h);
    std::lock_guard<std::mutex> lock(g_mu);
    auto it = g_loaded.find(h);
    if (it != g_loaded.end()) {
        ++it->second.users;
        *func_out = it->second.func;
        return WB_OK;
    }
    char name[40];
    snprintf(name, sizeof(name), "%016llx.co", (unsigned long long)h);
    const std::string dir = cache_dir(), path = dir.empty() ? std::string() : dir + "/" + name;
    std::vector<char> code;
    if (path.empty() || !read_file(path, code) || !plausible_code_object(path, code)) {
        std::string log;
        const int rc = compile(src, prop.gcnArchName, code, log);
        if (rc != WB_OK) {
            wb_set_error("wb_model_specialize: %.400s", log.c_str());
            return rc;
        }
        if (!path.empty()) write_file_atomic(dir, path, code);
    }
    JitKernel k;
    hipError_t e = hipModuleLoadData(&k.module, code.data());
    if (e == hipSuccess) e = hipModuleGetFunction(&k.func, k.module, "wb_casc_jit");
    if (e != hipSuccess) {
        if (!path.empty()) (void)unlink(path.c_str());          // (a stale or damaged cache entry: compile again next time)
        wb_set_error("wb_model_specialize: loading the compiled kernel failed: %s", hipGetErrorString(e));
        return WB_ERR_HIP;
    }
    k.users = 1;
    g_loaded[h] = k;
    evict_idle_modules();
    *func_out = k.func;
    return WB_OK;
}

// A model lets go of a specialised kernel (wb_model_destroy, a build that failed the self-test): its module becomes idle.
// It is not unloaded on the spot -- a hipGraph captured with the kernel may outlive the model by a moment (Python drops a
// scan state's model and graph in no particular order) -- but when the next module is loaded and more than
// WB_JIT_MODULES_MAX (64) are: the longest-idle one goes first, behind a device synchronisation.  A sweep over thousands
// of models (training, threshold search) stays bounded; a model that comes back within the window finds its kernel loaded.
void wb_jit_release(void *func) {
    if (!func) return;
    std::lock_guard<std::mutex> lock(g_mu);
    for (auto &kv : g_loaded) {
        if (kv.second.func != (hipFunction_t)func) continue;
        if (kv.second.users > 0 && --kv.second.users == 0) kv.second.released = ++g_release_clock;
        return;
    }
}

namespace {
// (g_mu held) unload idle modules, longest idle first, while more than the cap are loaded
void evict_idle_modules() {
    static const size_t cap = getenv("WB_JIT_MODULES_MAX") ? (size_t)atoi(getenv("WB_JIT_MODULES_MAX")) : 64;
    if (cap == 0) return;                                    // (0: never unload)
    bool synced = false;
    while (g_loaded.size() > cap) {
        auto victim = g_loaded.end();
        for (auto it = g_loaded.begin(); it != g_loaded.end(); ++it)
            if (it->second.users == 0 && (victim == g_loaded.end() || it->second.released < victim->second.released)) victim = it;
        if (victim == g_loaded.end()) return;                // (every module has a user)
        if (!synced) (void)hipDeviceSynchronize();           // (nothing of an idle module's last scans in flight)
        synced = true;
        (void)hipModuleUnload(victim->second.module);
        g_loaded.erase(victim);
    }
}
}  // namespace

// Compile check without a GPU (the CPU test suite): a synthetic cascade of n_stages random depth-`depth` trees through
// the same generator and hiprtc for `arch`.  Returns the code object's size in *code_bytes.
extern "C" int wb_jit_compile_check(int depth, int n_stages, const char *arch, int64_t *code_bytes) {
    return wb_jit_compile_check2(depth, n_stages, 1, arch, code_bytes);
}

extern "C" int wb_jit_compile_check2(int depth, int n_stages, int elem_bytes, const char *arch, int64_t *code_bytes) {
    return wb_jit_compile_check3(depth, n_stages, elem_bytes, 4, arch, code_bytes);
}

extern "C" int wb_jit_compile_check3(int depth, int n_stages, int elem_bytes, int rpw, const char *arch, int64_t *code_bytes) {
    WB_REQUIRE(wb_cascade_has_kernel(depth, rpw, 8), "wb_jit_compile_check: no tile kernel of %d rows per wave", rpw);
    WB_REQUIRE(depth >= 1 && depth <= WB_CASC_MAX_DEPTH && n_stages >= 1 && n_stages <= 4096 && arch && code_bytes &&
               (elem_bytes == 1 || elem_bytes == 2), "wb_jit_compile_check: bad argument");
    const int SD = WB_STAGE_DWORDS(depth), NI = WB_STAGE_NI(depth), NL = WB_STAGE_NL(depth), G = wb_cascade_group(depth);
    std::vector<int32_t> words((size_t)(n_stages + G) * SD, 0);
    uint32_t x = 12345u;
    auto rnd = [&]() { return x = x * 1664525u + 1013904223u; };
    for (int s = 0; s < n_stages + G; ++s) {
        int32_t *rec = words.data() + (size_t)s * SD;
        float *f = reinterpret_cast<float *>(rec);
        if (s >= n_stages) {
            f[2 * NI + NL] = -INFINITY;
            continue;
        }
        for (int i = 0; i < NI; ++i) {
            rec[i] = (int32_t)(rnd() % 3000u) * elem_bytes;
            rec[NI + i] = (int32_t)(rnd() % (elem_bytes == 2 ? 1000u : 255u));
        }
        for (int i = 0; i < NL; ++i) f[2 * NI + i] = (float)(rnd() % 2000u) * 1e-3f - 1.0f;
        f[2 * NI + NL] = s % 7 == 3 ? -INFINITY : -0.5f * (float)s;
    }
    // (as wb_model_create decides it: a stage table beyond 16 KiB is not mirrored in LDS)
    const int lds_stages = n_stages * SD * 4 <= 16 * 1024 ? n_stages : 0;
    std::vector<char> code;
    std::string log;
    const int rc = build_checked(make_source(words.data(), words.size(), n_stages, depth, rpw, 8, 4, rpw * 8 + 11, WB_CASC_TC + 12, elem_bytes, lds_stages),
                                 arch, code, log);
    if (rc != WB_OK) {
        wb_set_error("wb_jit_compile_check: %.400s", log.c_str());
        return rc;
    }
    *code_bytes = (int64_t)code.size();
    return WB_OK;
}

// A specialised kernel is run-time compiled code for ONE model: before it is trusted it scans a synthetic two-level
// pyramid of byte tiles several times and must give, every time, exactly what the generic kernel of the library gives on
// the same bytes: per-stage alive counts and the detection records (window, score bits).  The levels hold tiles of every
// kind the kernel distinguishes -- regions of different byte statistics, so that under most cascades some tiles keep more
// windows than the capped queue holds, some a few hundred, some a handful --, a ragged right and bottom edge, and a level
// of a single partial tile.  (hiprtc's code for some cascades of depth-3 trees has given wrong records on nine scans of
// ten: profiles/r04/jit_selftest.txt.)  A kernel that fails is not used: WB_ERR_UNSUPPORTED, the model stays on the
// generic kernel.  WB_JIT_SELFTEST=<passes> (default 6; 0 = skip the test).
int wb_jit_selftest(WbModel *model, int chn_dtype, WbFormRecords *rec) {
    static const int passes = getenv("WB_JIT_SELFTEST") ? atoi(getenv("WB_JIT_SELFTEST")) : 6;
    if (passes <= 0) return WB_OK;
    // (the levels in units of the form's own tile; the table in the model's units, whole, as any caller may hand it over)
    const int eb = rec->elem_bytes, C = model->C, m = model->m, n = model->n, T = model->n_stages, TR = rec->tile_rows, unit = model->tile_rows;
    struct Lv { int gh, gw; } lv[2] = {{2 * TR + TR / 2 + 1, 64 + 37}, {TR / 2 - 3 > 0 ? TR / 2 - 3 : 1, 24}};
    std::vector<WbLevel> levels(2);
    std::vector<WbTile> tiles;
    int64_t elems = 0, windows = 0;
    for (int l = 0; l < 2; ++l) {
        memset(&levels[l], 0, sizeof(WbLevel));
        levels[l].u = lv[l].gh + m;
        levels[l].v = lv[l].gw + n;
        levels[l].chn_off = elems;
        elems += (int64_t)levels[l].u * levels[l].v * C;
        windows += (int64_t)lv[l].gh * lv[l].gw;
        for (int ty = 0; ty * unit < lv[l].gh; ++ty)
            for (int tx = 0; tx * 64 < lv[l].gw; ++tx) tiles.push_back(WbTile{l, (uint16_t)ty, (uint16_t)tx});
    }
    // bytes: four kinds of 16 x 16 regions (the whole range, dark, middle, bright), LCG noise inside
    std::vector<uint8_t> host((size_t)elems * eb + 16, 0);
    uint32_t x = 2463534242u;
    for (int l = 0; l < 2; ++l)
        for (int r = 0; r < levels[l].u; ++r)
            for (int c = 0; c < levels[l].v; ++c)
                for (int ch = 0; ch < C; ++ch) {
                    x = x * 1664525u + 1013904223u;
                    const int kind = ((r >> 4) + 2 * (c >> 4) + l) & 3;
                    const uint32_t lo = kind == 0 ? 0u : kind == 1 ? 0u : kind == 2 ? 100u : 200u, span = kind == 0 ? 256u : kind == 1 ? 32u : kind == 2 ? 60u : 56u;
                    const uint32_t v = (lo + (x >> 16) % span) * (eb == 2 ? 3u : 1u);
                    const size_t at = (size_t)levels[l].chn_off + ((size_t)r * levels[l].v + c) * C + ch;
                    if (eb == 1) host[at] = (uint8_t)v;
                    else memcpy(&host[at * 2], &v, 2);
                }
    const uint32_t cap = (uint32_t)windows;                  // per shard: every window of the pyramid may survive in one
    uint8_t *chn = nullptr;
    WbLevel *d_levels = nullptr;
    WbTile *d_tiles = nullptr;
    WbDet *det = nullptr;
    uint32_t *ctr = nullptr;                                 // [WB_DET_SHARDS] counts, then alive [2][T]
    const size_t ctr_words = WB_DET_SHARDS + 2 * (size_t)T;
    hipStream_t st = nullptr;
    auto cleanup = [&]() {
        if (st) (void)hipStreamDestroy(st);
        (void)hipFree(chn); (void)hipFree(d_levels); (void)hipFree(d_tiles); (void)hipFree(det); (void)hipFree(ctr);
    };
#define WB_ST_CHECK(expr)                                                                            \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) {                                                                      \
            wb_set_error("wb_model_specialize (self-test): %s: %s", #expr, hipGetErrorString(e_));   \
            cleanup();                                                                               \
            return WB_ERR_HIP;                                                                       \
        }                                                                                            \
    } while (0)
    WB_ST_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    WB_ST_CHECK(hipMalloc(&chn, host.size()));
    WB_ST_CHECK(hipMalloc(&d_levels, levels.size() * sizeof(WbLevel)));
    WB_ST_CHECK(hipMalloc(&d_tiles, tiles.size() * sizeof(WbTile)));
    WB_ST_CHECK(hipMalloc(&det, (size_t)WB_DET_SHARDS * cap * sizeof(WbDet)));
    WB_ST_CHECK(hipMalloc(&ctr, ctr_words * 4));
    WB_ST_CHECK(hipMemcpyAsync(chn, host.data(), host.size(), hipMemcpyHostToDevice, st));
    WB_ST_CHECK(hipMemcpyAsync(d_levels, levels.data(), levels.size() * sizeof(WbLevel), hipMemcpyHostToDevice, st));
    WB_ST_CHECK(hipMemcpyAsync(d_tiles, tiles.data(), tiles.size() * sizeof(WbTile), hipMemcpyHostToDevice, st));
    struct Result {
        std::vector<uint32_t> ctr;
        std::vector<WbDet> det;
    };
    auto scan = [&](Result &out) -> int {
        hipError_t e = hipMemsetAsync(ctr, 0, ctr_words * 4, st);
        if (e != hipSuccess) return WB_ERR_HIP;
        const int rc = wb_cascade_launch(st, model, chn, chn_dtype, 0, 1, d_levels, 2, d_tiles, (int)tiles.size(), det, ctr, cap, ctr + WB_DET_SHARDS);
        if (rc != WB_OK) return rc;
        out.ctr.resize(ctr_words);
        e = hipMemcpyAsync(out.ctr.data(), ctr, ctr_words * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return WB_ERR_HIP;
        out.det.clear();
        for (int s = 0; s < WB_DET_SHARDS; ++s) {
            const uint32_t k = out.ctr[s] < cap ? out.ctr[s] : cap;
            const size_t at = out.det.size();
            out.det.resize(at + k);
            if (k && hipMemcpy(out.det.data() + at, det + (size_t)s * cap, (size_t)k * sizeof(WbDet), hipMemcpyDeviceToHost) != hipSuccess) return WB_ERR_HIP;
        }
        std::sort(out.det.begin(), out.det.end(), [](const WbDet &p, const WbDet &q) {
            if (p.level != q.level) return p.level < q.level;
            if (p.r != q.r) return p.r < q.r;
            return p.c < q.c;
        });
        return WB_OK;
    };
    Result want, got;
    void *const jf = rec->jit;
    rec->jit = nullptr;                                      // the generic kernel ...
    int rc = scan(want);
    rec->jit = jf;                                           // ... and the specialised one
    int bad = 0;
    uint64_t n_det = 0;
    for (int p = 0; rc == WB_OK && p < passes; ++p) {
        rc = scan(got);
        if (rc != WB_OK) break;
        bool same = got.det.size() == want.det.size() && memcmp(got.ctr.data() + WB_DET_SHARDS, want.ctr.data() + WB_DET_SHARDS, 2 * (size_t)T * 4) == 0;
        for (size_t i = 0; same && i < got.det.size(); ++i)
            same = got.det[i].level == want.det[i].level && got.det[i].r == want.det[i].r && got.det[i].c == want.det[i].c &&
                   memcmp(&got.det[i].score, &want.det[i].score, 4) == 0 && got.det[i].image == want.det[i].image;
        bad += !same;
        n_det = want.det.size();
        if (!same && getenv("WB_JIT_VERBOSE")) {              // the first records that differ, both sides
            int shown = 0;
            for (size_t i = 0; i < got.det.size() && i < want.det.size() && shown < 6; ++i) {
                const WbDet &g = got.det[i], &w = want.det[i];
                if (g.level == w.level && g.r == w.r && g.c == w.c && memcmp(&g.score, &w.score, 4) == 0) continue;
                fprintf(stderr, "[wb_jit] self-test pass %d, record %zu: specialised (level %d, r %d, c %d, score %.6g) generic (level %d, r %d, c %d, score %.6g)\n",
                        p, i, g.level, (int)g.r, (int)g.c, g.score, w.level, (int)w.r, (int)w.c, w.score);
                ++shown;
            }
            if (got.det.size() != want.det.size()) fprintf(stderr, "[wb_jit] self-test pass %d: %zu records against %zu\n", p, got.det.size(), want.det.size());
        }
    }
    cleanup();
#undef WB_ST_CHECK
    if (rc != WB_OK) {
        if (rc == WB_ERR_HIP) wb_set_error("wb_model_specialize (self-test): a HIP call failed");
        return rc;
    }
    if (getenv("WB_JIT_VERBOSE"))
        fprintf(stderr, "[wb_jit] self-test: %d of %d scans differ from the generic kernel (%llu windows, %llu detections)\n", bad, passes,
                (unsigned long long)windows, (unsigned long long)n_det);
    if (bad) {
        wb_set_error("wb_model_specialize: the specialised kernel disagreed with the generic kernel on %d of %d self-test scans; "
                     "the model stays on the generic kernel", bad, passes);
        return WB_ERR_UNSUPPORTED;
    }
    return WB_OK;
}
