// volume_kernels.h - kernels on whole volumes besides the packing ones of index_kernels.h: the gather of a subset of several volumes' reads into one
// (necat_volume_gather; the word function is volume_gather.h's, which g++ tests), and a volume's words back as pac bytes (necat_volume_download).
#pragma once
#include "volume_gather.h"

namespace necat {

// One thread per destination word, grid-strided; a word is written once, by one plain store.  HBM-bound: the subset's bytes are read once (a source word
// that two destination words share comes from the cache the second time) and written once; the offsets of the binary search are a few KB to MB that stay cached.
__global__ void __launch_bounds__(256)
k_vol_gather(const u64* __restrict__ dst_off, const u64* __restrict__ src_off, const u32* __restrict__ src_vol, u64 n, const u64* const* __restrict__ vol_words,
             u64 nwords, u64* __restrict__ out)
{
    const u64 nthreads = (u64)gridDim.x * blockDim.x;
    for (u64 w = (u64)blockIdx.x * blockDim.x + threadIdx.x; w < nwords; w += nthreads) out[w] = vgather::gather_word(w, dst_off, src_off, src_vol, n, vol_words);
}

// k_repack the other way: little-endian 2-bit words -> the 8 pac bytes each holds
__global__ void __launch_bounds__(256)
k_unpack_words(const u64* __restrict__ words, u64 nwords, u64* __restrict__ pac_words)
{
    const u64 nthreads = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < nwords; i += nthreads) pac_words[i] = vgather::swap_fields(words[i]);
}

}  // namespace necat
