// k_varlen.h - a batch of reads of mixed lengths bucketed by length on the device (mc_search_varlen): the fixed-length pipeline
// then runs once per bucket, each bucket's reads back to back at that bucket's pitch.
//   k_vl_hist     per tile of MC_VL_TILE reads: how many reads of each length; counts[len * ntiles + tile]
//   k_bin_scan    one workgroup: exclusive scan of counts in that (length-major) order -> where each tile's reads of each length go;
//                 start[len] = first sorted position of the bucket of length len, start[nbins] = n.  The one scan of every (bin, tile)
//                 count table: k_classes.h launches it with its own number of bins
//   k_vl_scatter  perm[sorted position] = read index; stable: within a bucket the read indices ascend
//   k_vl_gather   each read's bases to its bucket's block of dst (byte_off[len] + rank in the bucket * len)
// The host has checked every length (1 .. MC_MAXAA * 3) before these run: off[i + 1] - off[i] is always a valid bin.
#pragma once

#define MC_VL_BINS 512
#define MC_VL_TILE 4096
#define MC_VL_BS 256

__global__ void __launch_bounds__(MC_VL_BS) k_vl_hist(const int64_t *__restrict__ off, int64_t n, uint32_t ntiles, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t hist[MC_VL_BINS];
    for (int i = threadIdx.x; i < MC_VL_BINS; i += MC_VL_BS) hist[i] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * MC_VL_TILE;
    for (int k = threadIdx.x; k < MC_VL_TILE; k += MC_VL_BS) {
        const int64_t i = base + k;
        if (i < n) atomicAdd(&hist[(int)(off[i + 1] - off[i])], 1u);
    }
    __syncthreads();
    for (int l = threadIdx.x; l < MC_VL_BINS; l += MC_VL_BS) counts[(size_t)l * ntiles + blockIdx.x] = hist[l];
}

// one workgroup of 1024 threads; m = nbins * ntiles entries, total n < 2^31
__global__ void __launch_bounds__(1024) k_bin_scan(uint32_t *__restrict__ counts, uint32_t m, uint32_t ntiles, uint32_t nbins, uint32_t *__restrict__ start)
{
    __shared__ uint32_t part[1024];
    const uint32_t t = threadIdx.x, chunk = (m + 1023) / 1024;
    const uint32_t lo = min(m, t * chunk), hi = min(m, lo + chunk);
    uint32_t s = 0;
    for (uint32_t i = lo; i < hi; i++) s += counts[i];
    part[t] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {                    // inclusive scan of the chunk sums (Hillis - Steele)
        const uint32_t v = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = part[t] - s;
    for (uint32_t i = lo; i < hi; i++) {
        const uint32_t v = counts[i];
        if (i % ntiles == 0) start[i / ntiles] = run;
        counts[i] = run;
        run += v;
    }
    if (t == 1023) start[nbins] = part[1023];
}

__global__ void __launch_bounds__(MC_VL_BS) k_vl_scatter(const int64_t *__restrict__ off, int64_t n, uint32_t ntiles, const uint32_t *__restrict__ tile_off, uint32_t *__restrict__ perm)
{
    __shared__ uint32_t cnt[MC_VL_BINS];
    __shared__ uint16_t slen[MC_VL_BS];
    for (int i = threadIdx.x; i < MC_VL_BINS; i += MC_VL_BS) cnt[i] = 0;
    const int t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * MC_VL_TILE;
    for (int r = 0; r < MC_VL_TILE / MC_VL_BS; r++) {
        const int64_t i = base + r * MC_VL_BS + t;
        const int len = i < n ? (int)(off[i + 1] - off[i]) : 0xFFFF;
        slen[t] = (uint16_t)len;
        __syncthreads();                                           // (also orders the previous round's cnt updates before these reads)
        if (i < n) {
            uint32_t rank = 0;
            for (int j = 0; j < t; j++) rank += slen[j] == (uint16_t)len;
            perm[tile_off[(size_t)len * ntiles + blockIdx.x] + cnt[len] + rank] = (uint32_t)i;
        }
        __syncthreads();
        if (i < n) atomicAdd(&cnt[len], 1u);
    }
}

// a wave per sorted position, striding over them: the grid is bounded (MC_VL_GATHER_BLOCKS workgroups), whatever the batch
#define MC_VL_GATHER_BLOCKS 65536
__global__ void __launch_bounds__(MC_VL_BS) k_vl_gather(const uint8_t *__restrict__ bases, const int64_t *__restrict__ off, const uint32_t *__restrict__ perm, int64_t n,
                                                        const uint32_t *__restrict__ start, const int64_t *__restrict__ byte_off, uint8_t *__restrict__ dst)
{
    const int64_t stride = (int64_t)gridDim.x * (MC_VL_BS / 64);
    for (int64_t p = (int64_t)blockIdx.x * (MC_VL_BS / 64) + (threadIdx.x >> 6); p < n; p += stride) {
        const uint32_t i = perm[p];
        const int64_t a = off[i];
        const int len = (int)(off[i + 1] - a);
        uint8_t *d = dst + byte_off[len] + (p - (int64_t)start[len]) * len;
        for (int k = mc_lane(); k < len; k += 64) d[k] = bases[a + k];
    }
}
