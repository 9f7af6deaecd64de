// The float32 -> uint8 rule of a baked texture, shared by the PNG encoder's float path (t4d_png.hip) and t4d_texture_quantize
// (t4d_texfinish.hip), so that both produce the bytes the reference's write_texture saves.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

// numpy's float32 -> uint8 cast on x86-64: truncate toward zero to int32 (cvttss2si: NaN and |y| >= 2^31 give INT_MIN), keep the
// low byte.  A multiply alone: nothing to contract.
__device__ __forceinline__ uint32_t t4d_quant_u8(float x)
{
    const float y = x * 255.0f;
    if (!(fabsf(y) < 2147483648.0f)) return 0u;
    return (uint32_t)(int32_t)y & 0xFFu;
}
