// The per-sample expressions of the band above 8 kHz that the offline join (highband.hip) and the stream
// pool's join (stream_highband.hip, section 3r) share: one source, so a streamed session is bit for bit the offline result.
#pragma once

// up_y + G (x - up_x); G = 1 ("keep") adds the band as it is
template <bool FOLLOW>
__device__ __forceinline__ float hb_mix(float upy, float upx, float x, float G) {
    const float hb = x - upx;
    return FOLLOW ? fmaf(G, hb, upy) : upy + hb;
}

// ((D - c) ga + c gb) / D, 0 <= c < D <= 128 * 640: c and D - c are exact in fp32, so the result carries three roundings
// however far apart the two gains lie
__device__ __forceinline__ float hb_lerp(float ga, float gb, unsigned c, unsigned D) {
    return fmaf(gb, (float)c, ga * (float)(D - c)) / (float)D;
}
