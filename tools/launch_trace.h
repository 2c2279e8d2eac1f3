// launch_trace.h -- shim of the launch-trace programs (tools/mfma_launch_trace.hip, tools/gemm_launch_trace.hip): force-included in front of the
// units of csrc/, it turns their kernel launches, LDS reservations and device allocations into records on the host, so that the host side of a path
// (set-up, the resolvers, the launchers) runs and can be compared between two versions of csrc/ on a machine without a GPU.  Each program defines
// the qoc_trace_* functions it is declared to need; the build commands are in the programs.
//
// -DQOC_TRACE_STREAMS (the GEMM program) also fakes what a host with streams of its own uses: stream / event creation and destruction (handles are
// numbers in creation order, the engine's stream is 0), event record / wait and memsets as trace lines, a device of 256 compute units, and
// synchronisation / error queries that succeed.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <type_traits>

struct QocTraceArg {
    enum Kind { INT, PTR, STRUCT } kind;
    long long i;               // INT
    const void* p;             // PTR: the pointer; STRUCT: the argument itself (valid during the call)
    size_t size;               // STRUCT: sizeof
};
// defined in the program
hipError_t qoc_trace_launch(const void* kernel, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const QocTraceArg* args, int count);
hipError_t qoc_trace_reserve(const void* kernel, int bytes);
hipError_t qoc_trace_malloc(void** p, size_t bytes);

static inline hipError_t qoc_trace_reserve3(const void* kernel, hipFuncAttribute, int bytes) { return qoc_trace_reserve(kernel, bytes); }

template <class T> static inline QocTraceArg qoc_trace_arg(const T& v) {
    if constexpr (std::is_null_pointer_v<T>) return {QocTraceArg::PTR, 0, nullptr, 0};
    else if constexpr (std::is_pointer_v<T>) return {QocTraceArg::PTR, 0, (const void*)v, 0};
    else if constexpr (std::is_integral_v<T>) return {QocTraceArg::INT, (long long)v, nullptr, 0};
    else return {QocTraceArg::STRUCT, 0, (const void*)&v, sizeof(T)};
}
template <class... A>
static inline hipError_t qoc_trace_launch_args(const void* kernel, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const A&... a) {
    const QocTraceArg args[] = {qoc_trace_arg(a)...};
    return qoc_trace_launch(kernel, grid, block, lds, stream, args, (int)sizeof...(A));
}

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) \
    ((void)qoc_trace_launch_args((const void*)(kernel), dim3(grid), dim3(block), lds, (hipStream_t)(stream), __VA_ARGS__))
// (the calls with an argument array that csrc/ has had: kernels of (QocDev, QocMfma))
#define hipLaunchKernel(kernel, grid, block, kargs, lds, stream) \
    qoc_trace_launch_args((const void*)(kernel), dim3(grid), dim3(block), lds, (hipStream_t)(stream), *(const QocDev*)(kargs)[0], *(const QocMfma*)(kargs)[1])
#define hipFuncSetAttribute(...) qoc_trace_reserve3(__VA_ARGS__)            // (variadic: template arguments bring commas of their own)
#define hipMalloc(p, bytes) qoc_trace_malloc((void**)(p), (bytes))
#define hipMemcpy(dst, src, bytes, kind) (memcpy((dst), (src), (bytes)), hipSuccess)

#ifndef QOC_TRACE_STREAMS
#define hipMemset(p, value, bytes) (((value) != 0 ? (void)memset((p), (value), (bytes)) : (void)0), hipSuccess)       // (allocations come zeroed)
#else
// defined in the program.  words > 0: a stream with a CU mask
hipError_t qoc_trace_stream_create(hipStream_t* s, unsigned words, const uint32_t* mask);
hipError_t qoc_trace_event_create(hipEvent_t* e);
hipError_t qoc_trace_destroy(const char* what, const void* handle);
hipError_t qoc_trace_event(const char* what, hipEvent_t e, hipStream_t s);
hipError_t qoc_trace_memset(void* p, int value, size_t bytes, hipStream_t s, bool async);

#define hipStreamCreateWithFlags(s, flags) qoc_trace_stream_create((s), 0, nullptr)
#define hipExtStreamCreateWithCUMask(s, words, mask) qoc_trace_stream_create((s), (words), (mask))
#define hipEventCreateWithFlags(e, flags) qoc_trace_event_create(e)
#define hipStreamDestroy(s) qoc_trace_destroy("stream", (const void*)(s))
#define hipEventDestroy(e) qoc_trace_destroy("event", (const void*)(e))
#define hipEventRecord(e, s) qoc_trace_event("record", (e), (hipStream_t)(s))
#define hipStreamWaitEvent(s, e, flags) qoc_trace_event("wait", (e), (hipStream_t)(s))
#define hipMemsetAsync(p, value, bytes, s) qoc_trace_memset((p), (value), (bytes), (hipStream_t)(s), true)
#define hipMemset(p, value, bytes) qoc_trace_memset((p), (value), (bytes), nullptr, false)
#define hipGetDevice(dev) (*(dev) = 0, hipSuccess)
#define hipDeviceGetAttribute(value, attribute, dev) (*(value) = 256, hipSuccess)
#define hipStreamSynchronize(s) ((void)(s), hipSuccess)
#define hipGetLastError() hipSuccess
#endif
