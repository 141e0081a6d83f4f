// sum_scale.inc -- the exact forms' sum scale: k_sum_scale_init and k_sum_scale (records or
// voxels).
// Included in the anonymous namespace of uampath.hip; relies on k2h.inc (X_E_MIN, x_word_exp,
// x_word_flags).

// uam_raster_sum_scale: scale = {e_phi, e_psi, flags, 0} of a record raster, flags = the phi
// words' side flags | the psi words' << 3.  Integer maxima and ORs only, so the words do not
// depend on the reduction's order: k_sum_scale_init writes the neutral words, then every wave
// of k_sum_scale folds its cells (a grid-stride loop) and issues one atomic per word.
// V: the cell -- a raster's 16-B record {phi, psi_nfz, ...} (uint4) or a volume's 8-B voxel
// {risk, psi_nfz} (uint2, uam_volume_sum_scale); the two fields are its first two words.
__global__ void k_sum_scale_init(int32_t* __restrict__ scale) {
    if (threadIdx.x < 4) scale[threadIdx.x] = threadIdx.x < 2 ? X_E_MIN : 0;
}
template <typename V>
__global__ __launch_bounds__(256) void k_sum_scale(const V* __restrict__ rec, int64_t cells,
                                                   int32_t* __restrict__ scale) {
    int32_t ec = X_E_MIN, en = X_E_MIN;
    uint32_t fl = 0;
    // 64 B of loads in flight per lane (past the end: the last cell again)
    constexpr int U = 64 / (int)sizeof(V);
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t c0 = (int64_t)blockIdx.x * 256 + threadIdx.x; c0 < cells; c0 += step * U) {
        V r[U];
#pragma unroll
        for (int k = 0; k < U; ++k) r[k] = rec[min(c0 + k * step, cells - 1)];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            ec = max(ec, x_word_exp(r[k].x));
            en = max(en, x_word_exp(r[k].y));
            fl |= x_word_flags(r[k].x) | (x_word_flags(r[k].y) << 3);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ec = max(ec, __shfl_xor(ec, o));
        en = max(en, __shfl_xor(en, o));
        fl |= (uint32_t)__shfl_xor((int32_t)fl, o);
    }
    if ((threadIdx.x & 63) == 0) {
        if (ec > X_E_MIN) atomicMax(scale + 0, ec);
        if (en > X_E_MIN) atomicMax(scale + 1, en);
        if (fl) atomicOr(scale + 2, (int32_t)fl);
    }
}
