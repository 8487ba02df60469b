// The attenuation limit (atten.py): the per-sample expressions every route shares -- enhance's ragged
// blend, AudioStream's rows and the stream pool's dry line (atten.hip) -- one source, so a limit means the same everywhere.
#pragma once

// out = y + g (x - y): y the wet (enhanced) sample, x the dry one, g = 10^(-L / 20) in [0, 1].  One subtraction and one
// fused multiply-add; g = 0 (no limit) returns y itself, whatever x holds.
__device__ __forceinline__ float atten_blend(float y, float x, float g) {
    return g == 0.f ? y : fmaf(g, x - y, y);
}

// the gain of sample i < 128 of the hop over which a session's limit moves: g_old + (g_new - g_old) (i + 1) / 128;
// (i + 1) / 128 is exact in fp32, and the last sample lands on g_new itself
__device__ __forceinline__ float atten_ramp(float g_old, float g_new, int i) {
    return i >= 127 ? g_new : fmaf(g_new - g_old, (float)(i + 1) * (1.f / 128.f), g_old);
}
