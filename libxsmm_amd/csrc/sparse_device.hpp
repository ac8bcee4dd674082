// sparse_device.hpp -- the few device-side names sparse_kernels.hip and bcsc_kernels.hip share.
#pragma once
#include <hip/hip_runtime.h>

namespace xamd {

// kernel-argument-block pointers are generic to the compiler; everything dereferenced here is global memory
#define GM __attribute__((address_space(1)))
typedef __attribute__((address_space(3))) void* lds_ptr_t;

typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef short bf16x8v __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4v __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2v __attribute__((ext_vector_type(2)));

}  // namespace xamd
