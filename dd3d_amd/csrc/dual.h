// Dual numbers {value, tangent} for the forward-mode derivatives of loss_grads.hip, and the Du overloads of the scalar operations in
// which box3d_decode.h and loss_common.h state the decode, the corners and GIoU (their float overloads are in box3d_decode.h).  A value
// part is the float operation itself, so the value of a Du instantiation is the float instantiation's, bit for bit.
// Conventions at the non-smooth points are torch's: min / max pass the gradient to the smaller / larger operand and split a tie in
// halves, clamp passes 1 on its closed interval, sqrt and the norms have derivative 0 at 0.
// The including translation unit turns floating-point contraction off before this header.
#pragma once
#include <math.h>

namespace dd3d {

struct Du {
  float v, d;
};
__device__ __forceinline__ Du operator+(Du a, Du b) { return {a.v + b.v, a.d + b.d}; }
__device__ __forceinline__ Du operator+(Du a, float b) { return {a.v + b, a.d}; }
__device__ __forceinline__ Du operator+(float a, Du b) { return {a + b.v, b.d}; }
__device__ __forceinline__ Du operator-(Du a, Du b) { return {a.v - b.v, a.d - b.d}; }
__device__ __forceinline__ Du operator-(Du a, float b) { return {a.v - b, a.d}; }
__device__ __forceinline__ Du operator-(float a, Du b) { return {a - b.v, 0.f - b.d}; }
__device__ __forceinline__ Du operator*(Du a, Du b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
__device__ __forceinline__ Du operator*(Du a, float b) { return {a.v * b, a.d * b}; }
__device__ __forceinline__ Du operator*(float a, Du b) { return {a * b.v, a * b.d}; }
__device__ __forceinline__ Du operator/(Du a, Du b) {
  const float q = a.v / b.v;
  return {q, (a.d - q * b.d) / b.v};
}
__device__ __forceinline__ Du operator/(Du a, float b) { return {a.v / b, a.d / b}; }
__device__ __forceinline__ Du operator/(float a, Du b) {
  const float q = a / b.v;
  return {q, (0.f - q * b.d) / b.v};
}

__device__ __forceinline__ float op_value(Du a) { return a.v; }
__device__ __forceinline__ Du op_sqrt(Du a) {  // derivative 0 at 0: torch's norm backward
  const float s = sqrtf(a.v);
  return {s, a.v > 0.f ? a.d / (2.0f * s) : 0.f};
}
__device__ __forceinline__ Du op_sqrt_positive(Du a) { return a.v > 0.f ? op_sqrt(a) : Du{0.f, 0.f}; }
__device__ __forceinline__ Du op_clamp_min(Du a, float m) { return {fmaxf(a.v, m), a.v >= m ? a.d : 0.f}; }  // x.clamp(min=m): 1 at equality
__device__ __forceinline__ Du op_clamp(Du a, float lo, float hi) { return {fminf(fmaxf(a.v, lo), hi), (a.v >= lo && a.v <= hi) ? a.d : 0.f}; }
__device__ __forceinline__ Du op_max(Du a, float b) {  // torch.max(a, b): a tie splits in halves
  return {fmaxf(a.v, b), a.v > b ? a.d : (a.v == b ? 0.5f * a.d : 0.f)};
}
__device__ __forceinline__ Du op_min(Du a, float b) { return {fminf(a.v, b), a.v < b ? a.d : (a.v == b ? 0.5f * a.d : 0.f)}; }
__device__ __forceinline__ Du op_tanh(Du a) {
  const float t = tanhf(a.v);
  return {t, (1.0f - t * t) * a.d};
}

}  // namespace dd3d
