// nan_math.hpp — max / min / clamp / ReLU as jnp.maximum, jnp.minimum, jnp.clip and torch.relu compute them: a NaN operand gives NaN
// (fmaxf / fminf return the OTHER operand: a diverged network would come out as ordinary numbers), -0 < +0.  IEEE 754-2019 maximum /
// minimum: one v_maximum3_f32 / v_minimum3_f32 on gfx950, the cost of the v_max_f32 / v_min_f32 they replace; on ordered operands the
// same value as fmaxf / fminf.  DESIGN.md, "Non-finite values".
#pragma once

__device__ __forceinline__ float max_nan(float a, float b) { return __builtin_elementwise_maximum(a, b); }
__device__ __forceinline__ float min_nan(float a, float b) { return __builtin_elementwise_minimum(a, b); }
__device__ __forceinline__ float clamp_nan(float x, float lo, float hi) { return min_nan(max_nan(x, lo), hi); }
__device__ __forceinline__ float relu_nan(float z) { return max_nan(z, 0.0f); }
