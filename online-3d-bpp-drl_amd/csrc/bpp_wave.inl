// bpp_wave.inl -- the wave-level primitives of the policy heads, the statistics kernels and the three searches, included by
// bpp_kernels.hip inside its anonymous namespace before bpp_heads.inl.  (The step, refill and runtime-geometry kernels keep the
// shuffles they were tuned with: bpp_tile_body.inl, bpp_tile_kernel.inl, bpp_rt_kernels.inl, bpp_stream_gen.inl.)

// ---- wave-wide reductions: the xor butterfly 32 .. 1, every lane ends with the result ------------------------------------
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m, kWave));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, kWave));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, kWave));
    return v;
}

// The wave's argmax of per-lane candidates (best, bi) under numpy's tie rules: the first maximum (np.argmax) or, with
// `last`, the last one (argsort()[-1]).  A lane's own scan keeps its first / last maximum the same way before it calls this.
__device__ __forceinline__ void wave_argmax(float &best, int &bi, bool last) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ob = __shfl_xor(best, m, kWave);
        const int oi = __shfl_xor(bi, m, kWave);
        if (ob > best || (ob == best && (last ? oi > bi : oi < bi))) best = ob, bi = oi;
    }
}

// The wave's smallest key and the value its lane holds (keys distinct, or equal keys with equal values).
__device__ __forceinline__ void wave_min_keyed(int &key, float &val) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const int ok = __shfl_xor(key, m, kWave);
        const float ov = __shfl_xor(val, m, kWave);
        if (ok < key) key = ok, val = ov;
    }
}

// Inclusive prefix sum over every group of WIDTH consecutive lanes (Hillis-Steele: d = 1, 2, ..., WIDTH / 2; `lane` is the
// lane's index in its group).  The float form adds in exactly this order: a CDF built on it depends on it.
template <int WIDTH = 64, typename T>
__device__ __forceinline__ T wave_scan_incl(T v, int lane) {
#pragma unroll
    for (int d = 1; d < WIDTH; d <<= 1) {
        const T o = __shfl_up(v, d, WIDTH);
        if (lane >= d) v += o;
    }
    return v;
}

// ---- the 16-lane DPP row: row_ror:n rotates within every 16-lane row; row_shr:n shifts, lanes without a source read 0 ------
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v, float old) {
    (void)old;
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v, int old) {
    (void)old;
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true);
}
__device__ __forceinline__ float row16_max(float v) {
    v = fmaxf(v, dpp_f<0x128>(v, v)); v = fmaxf(v, dpp_f<0x124>(v, v)); v = fmaxf(v, dpp_f<0x122>(v, v)); v = fmaxf(v, dpp_f<0x121>(v, v));
    return v;
}
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_f<0x128>(v, v); v += dpp_f<0x124>(v, v); v += dpp_f<0x122>(v, v); v += dpp_f<0x121>(v, v);
    return v;
}
__device__ __forceinline__ int row16_min(int v) {
    v = min(v, dpp_i<0x128>(v, v)); v = min(v, dpp_i<0x124>(v, v)); v = min(v, dpp_i<0x122>(v, v)); v = min(v, dpp_i<0x121>(v, v));
    return v;
}
__device__ __forceinline__ int row16_isum(int v) {
    v += dpp_i<0x128>(v, v); v += dpp_i<0x124>(v, v); v += dpp_i<0x122>(v, v); v += dpp_i<0x121>(v, v);
    return v;
}
__device__ __forceinline__ float row16_scan(float v) {   // inclusive prefix sum along the row
    v += dpp_f<0x111>(v, 0.0f); v += dpp_f<0x112>(v, 0.0f); v += dpp_f<0x114>(v, 0.0f); v += dpp_f<0x118>(v, 0.0f);
    return v;
}
