// catan_abi_base.h - what every host file of catan_abi.hip needs and no handle: the error string, the checks, the launch arithmetic, the tail
// of a counter read, staged device allocations.  The host files (this one, catan_abi_nn_launch.h, catan_abi_hooks.h, catan_abi_nn.h,
// catan_abi_players.h) are pieces of that one translation unit, included behind its kernel files; none of them stands alone.
#pragma once

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define HIPCHK(x)                                                                                    \
    do {                                                                                             \
        hipError_t e_ = (x);                                                                         \
        if (e_ != hipSuccess) return fail(CATAN_EHIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
    } while (0)
#define OK_OR_RETURN(x) do { int r_ = (x); if (r_ != CATAN_OK) return r_; } while (0)   // ... and for the helpers that return a CATAN_* code themselves
static int launched() { HIPCHK(hipGetLastError()); return CATAN_OK; }                    // the end of a call that launched kernels
// fn<__hip_bfloat16>(...) or fn<float>(...) by an entry point's is_bf16
#define BY_DTYPE(is_bf16, fn, ...) ((is_bf16) ? fn<__hip_bfloat16>(__VA_ARGS__) : fn<float>(__VA_ARGS__))

static inline hipStream_t S(catan_stream_t s) { return (hipStream_t)s; }
static inline unsigned blocks(long n, int b) { return (unsigned)((n + b - 1) / b); }
// ... and at most `cap` of them: the grid of a kernel that strides over the rest
static inline unsigned grid_for(long total, long per_block, long cap) {
    const long nb = (total + per_block - 1) / per_block;
    return (unsigned)(nb < cap ? nb : cap);
}

// The tail of every counter read: the block to the host, zeroed behind the copy if `reset`, and the stream waited for
static int read_counters(uint64_t* out_host, unsigned long long* dev, size_t bytes, int reset, hipStream_t st) {
    HIPCHK(hipMemcpyAsync(out_host, dev, bytes, hipMemcpyDeviceToHost, st));
    if (reset) HIPCHK(hipMemsetAsync(dev, 0, bytes, st));
    HIPCHK(hipStreamSynchronize(st));
    return CATAN_OK;
}

// The device allocations of a call that builds something beside what is in use and installs it only when all of it stands.  Nothing is
// tried after the first failure (rc); what the call has not committed is freed when it returns, whichever way it returns.
namespace {                                      // (its members stay out of the library's exported symbols)
struct Staged {
    hipError_t rc = hipSuccess;
    std::vector<void*> held;
    template <class T>
    void alloc(T*& p, size_t bytes) {
        if (rc != hipSuccess) return;
        rc = hipMalloc((void**)&p, bytes);
        if (rc == hipSuccess) held.push_back(p); else p = nullptr;
    }
    bool ok() const { return rc == hipSuccess; }
    int enomem(const char* fn) const { return fail(CATAN_ENOMEM, std::string(fn) + ": hipMalloc: " + hipGetErrorString(rc)); }
    void free_now(void* p) {                     // a scratch word the call is done with
        for (void*& h : held) if (h == p) { hipFree(p); h = held.back(); held.pop_back(); return; }
    }
    void commit() { held.clear(); }              // the caller has installed every pointer
    ~Staged() { for (void* p : held) hipFree(p); }
};
}  // namespace

extern "C" {

const char* catan_last_error(void) { return g_err.c_str(); }

#ifndef CATAN_BUILD_HASH_STR
#define CATAN_BUILD_HASH_STR "unhashed-build-0000000000000000"
#endif
// "CATAN_BUILD_HASH=" + the sha256 prefix of csrc/* and include/catan_hip.h the build script computed (_lib.source_hash):
// the marker makes it readable from the file without loading the library
static const char g_build_hash[] = "CATAN_BUILD_HASH=" CATAN_BUILD_HASH_STR;
const char* catan_build_hash(void) { return g_build_hash + 17; }

}  // extern "C"
