// mfma_launch_trace.h -- shim for tools/mfma_launch_trace.hip: force-included in front of the MFMA units, it turns their kernel launches, LDS
// reservations and device allocations into records on the host, so that the host side of the MFMA path (qoc_mfma_setup, the resolvers, the
// launchers) runs and can be compared between two versions of csrc/ on a machine without a GPU.  Build command: see mfma_launch_trace.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <type_traits>

struct QocTraceArg {
    enum Kind { INT, PTR, STRUCT } kind;
    long long i;               // INT
    const void* p;             // PTR: the pointer; STRUCT: the argument itself (valid during the call)
    size_t size;               // STRUCT: sizeof
};
// defined in mfma_launch_trace.hip
hipError_t qoc_trace_launch(const void* kernel, dim3 grid, dim3 block, size_t lds, const QocTraceArg* args, int count);
hipError_t qoc_trace_reserve(const void* kernel, int bytes);
hipError_t qoc_trace_malloc(void** p, size_t bytes);

static inline hipError_t qoc_trace_reserve3(const void* kernel, hipFuncAttribute, int bytes) { return qoc_trace_reserve(kernel, bytes); }

template <class T> static inline QocTraceArg qoc_trace_arg(const T& v) {
    if constexpr (std::is_null_pointer_v<T>) return {QocTraceArg::PTR, 0, nullptr, 0};
    else if constexpr (std::is_pointer_v<T>) return {QocTraceArg::PTR, 0, (const void*)v, 0};
    else if constexpr (std::is_integral_v<T>) return {QocTraceArg::INT, (long long)v, nullptr, 0};
    else return {QocTraceArg::STRUCT, 0, (const void*)&v, sizeof(T)};
}
template <class... A> static inline hipError_t qoc_trace_launch_args(const void* kernel, dim3 grid, dim3 block, size_t lds, const A&... a) {
    const QocTraceArg args[] = {qoc_trace_arg(a)...};
    return qoc_trace_launch(kernel, grid, block, lds, args, (int)sizeof...(A));
}

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) ((void)qoc_trace_launch_args((const void*)(kernel), dim3(grid), dim3(block), lds, __VA_ARGS__))
// (the calls with an argument array that csrc/ has had: kernels of (QocDev, QocMfma))
#define hipLaunchKernel(kernel, grid, block, kargs, lds, stream) \
    qoc_trace_launch_args((const void*)(kernel), dim3(grid), dim3(block), lds, *(const QocDev*)(kargs)[0], *(const QocMfma*)(kargs)[1])
#define hipFuncSetAttribute(...) qoc_trace_reserve3(__VA_ARGS__)            // (variadic: template arguments bring commas of their own)
#define hipMalloc(p, bytes) qoc_trace_malloc((void**)(p), (bytes))
#define hipMemcpy(dst, src, bytes, kind) (memcpy((dst), (src), (bytes)), hipSuccess)
#define hipMemset(p, value, bytes) (((value) != 0 ? (void)memset((p), (value), (bytes)) : (void)0), hipSuccess)       // (allocations come zeroed)
