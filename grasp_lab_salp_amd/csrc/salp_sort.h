// salp_sort.h — salp_sort.hip's two functions, internal to the library
// (salp_create and the lock-step launches of salp_kernels.hip call them).
#pragma once

#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

// Temporary storage bytes for sorting n (uint32 key, int32 id) pairs.
extern "C" __attribute__((visibility("hidden"))) hipError_t salp_sort_temp_bytes(int64_t n, size_t* bytes);

// keys (predicted ticks, < 2^16) descending, carrying the env ids into `order`.
extern "C" __attribute__((visibility("hidden"))) hipError_t salp_sort_launch(
    void* temp, size_t temp_bytes, const uint32_t* keys_in, uint32_t* keys_out, const int32_t* ids_in,
    int32_t* order, int64_t n, void* stream);
