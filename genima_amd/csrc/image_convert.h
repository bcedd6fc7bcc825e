// The byte -> half conversion of the image path, shared by every kernel that writes the trainer's f16 NHWC layout (elementwise.hip:
// image_u8_to_f16_kernel, gather_u8_to_f16_kernel; render.hip: render_spheres_kernel) so that their outputs agree bit for bit.
#pragma once
#include "common.h"

// ToTensor + Normalize of one byte
__device__ __forceinline__ f16 u8_to_f16_value(uint8_t v, float mul, float add) { return (f16)((float)v / 255.0f * mul + add); }
