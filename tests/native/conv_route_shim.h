// Forced include (-include) of the host-only builds of the conv launcher sources for tests/native/conv_route_harness.cpp: a kernel
// launch becomes a call of the harness's recorder, which sees the kernel's host stub and the ConvParams the kernel would receive.
#pragma once
#include <hip/hip_runtime.h>

extern "C" void frp_route_record_launch(const void* stub, unsigned grid, unsigned block, size_t lds, const void* params, size_t bytes);

template <class Kern, class Params>
static inline void frp_route_launch(Kern kern, dim3 grid, dim3 block, size_t lds, const Params& p) {
    frp_route_record_launch(reinterpret_cast<const void*>(kern), grid.x, block.x, lds, &p, sizeof(Params));
}

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kern, grid, block, lds, stream, ...) frp_route_launch(kern, grid, block, lds, __VA_ARGS__)
