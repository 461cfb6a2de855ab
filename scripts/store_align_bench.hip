// Diagnostic: HBM write rate of 16-byte global stores at byte misalignment,
// in the shape of pack_cs_kernel's tile copy-out: workgroup t (4 waves, 8 per
// CU) writes its tile of 10,512 bytes at out + 10512 t + m, every store
// instruction 1 KiB contiguous per wave, for m = 0 (aligned), 1, 4, 8, 15.
//   hipcc -O3 --offload-arch=gfx950 -o scripts/store_align_bench scripts/store_align_bench.hip
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 __attribute__((aligned(1))) u32x4_unaligned;

constexpr uint32_t kTileBytes = 10512;  // 657 blocks of 16 bytes
constexpr uint32_t kTiles = 65536;

__global__ void __launch_bounds__(256, 8) st(uint8_t* out, uint32_t m) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint8_t* dst = out + (uint64_t)blockIdx.x * kTileBytes + m;
    const uint32_t nb = kTileBytes / 16;
    const uint32_t k0 = nb * wave / 4, k1 = nb * (wave + 1) / 4;
    const u32x4 v = {blockIdx.x, lane, wave, m};
    for (uint32_t k = k0 + lane; k < k1; k += 64)
        *reinterpret_cast<u32x4_unaligned*>(dst + 16u * k) = v;
}

int main() {
    const size_t bytes = (size_t)kTiles * kTileBytes;
    uint8_t* d;
    if (hipMalloc(&d, bytes + 64) != hipSuccess) return 1;
    hipEvent_t a, b;
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
    const uint32_t mis[5] = {0, 1, 4, 8, 15};
    printf("16-byte stores, %u tiles of %u bytes (%.0f MB), 4 waves a tile, 8 tiles a CU\n", kTiles,
           kTileBytes, bytes / 1e6);
    for (int pass = 0; pass < 2; pass++) {
        for (uint32_t m : mis) {
            float t[7];
            for (int rep = 0; rep < 7; rep++) {
                (void)hipEventRecord(a);
                hipLaunchKernelGGL(st, dim3(kTiles), dim3(256), 0, 0, d, m);
                (void)hipEventRecord(b);
                (void)hipEventSynchronize(b);
                (void)hipEventElapsedTime(&t[rep], a, b);
            }
            std::sort(t + 2, t + 7);  // (the first two warm up)
            printf("pass %d  misalignment %2u: median %.1f us (min %.1f, max %.1f), %.0f GB/s\n",
                   pass, m, t[4] * 1e3, t[2] * 1e3, t[6] * 1e3, bytes / (t[4] * 1e-3) / 1e9);
        }
    }
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    (void)hipFree(d);
    return 0;
}
