// Host-side plumbing shared by the C ABIs of the six libraries: the per-thread error text behind *_last_error(), the
// launch check, the aligned bump allocator of the workspace carve-ups and the refusals of an aligned workspace.  Integer and
// host code only: no floating-point contraction setting reaches it.  Nothing here is exported: each library gets its own
// copy, shared by its translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#pragma GCC visibility push(hidden)
namespace capi {

inline thread_local char g_err[512] = "";

// formats the error text and returns `code`, the value the failing entry point returns
inline int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
inline int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// 0, or fail(code, "<what><sep><HIP's error text>") when one of the launches enqueued since the last check was refused
inline int check_launch(int code, const char* what, const char* sep = ": ") {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(code, "%s%s%s", what, sep, hipGetErrorString(e));
    return 0;
}

__host__ __device__ inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
__host__ __device__ inline int ceil_div(int x, int m) { return (x + m - 1) / m; }   // the workgroups of m threads that cover x items
inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) & ~(a - 1); }   // a: a power of two

// Carves a buffer into pieces in the order they are asked for, each starting on a multiple of `align` bytes.  A null base
// only counts the bytes: `off` is the size the buffer needs.
struct Bump {
    char* base;
    size_t align, off = 0;
    explicit Bump(void* b, size_t a = 256) : base(static_cast<char*>(b)), align(a) {}
    size_t reserve(size_t nbytes) { const size_t o = off; off += align_up(nbytes, align); return o; }   // offset of the piece
    template <class T = char>
    T* take(size_t nbytes) { const size_t o = reserve(nbytes); return base ? reinterpret_cast<T*>(base + o) : nullptr; }
};

// The refusals of a caller-provided workspace that must start on a 256-byte boundary and hold `need` bytes; 0 when it will do.
inline int check_workspace(const char* who, const void* workspace, size_t workspace_bytes, size_t need) {
    if (!workspace) return fail(-1, "%s: null workspace", who);
    if (reinterpret_cast<uintptr_t>(workspace) % 256) return fail(-1, "%s: workspace must be 256-byte aligned", who);
    if (workspace_bytes < need) return fail(-2, "%s: workspace too small: %zu < %zu bytes", who, workspace_bytes, need);
    return 0;
}

}  // namespace capi
#pragma GCC visibility pop
