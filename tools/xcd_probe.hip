// Which XCD runs block (x, y) of a 2-D grid whose gridDim.x is a multiple of 8?  The premise of MDC_OPT_XCD_ROTATE
// (csrc/xcd_placement.h): blocks with equal x % 8 run on ONE XCD in every frame group y, also behind blocks that exit at once
// (the padding slots of the placement table), so that shifting the table's columns by y shifts the tiles' XCDs.
// Every block reads its XCD's id (s_getreg_b32 on HW_REG_XCC_ID), one lane writes it with an ordinary store.  The grid is
// the headline's, 80 x 43 blocks of 1024 threads with its dynamic LDS (two workgroups per CU), the blocks stay for a while
// (unevenly), the padding blocks leave at once: in the columns of one XCD (5 of 80, as 75 tiles in bands of 10 leave them), in
// the columns the rotation moves them to (another XCD every group), or nowhere.
//   hipcc --offload-arch=gfx950 -O2 -o tools/bin/xcd_probe tools/xcd_probe.hip && tools/bin/xcd_probe [gx] [gy] [lds bytes] [busy us] [launches]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x)                                                                        \
  do {                                                                               \
    hipError_t e_ = (x);                                                             \
    if (e_ != hipSuccess) {                                                          \
      std::printf("%s failed: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__); \
      return 2;                                                                      \
    }                                                                                \
  } while (0)

// pad: 0 = no block exits early, 1 = entries 8 j + 7, j >= pad_from, are padding (fixed columns), 2 = the same entries read
// through the rotated mapping (x & ~7) | ((x + y) & 7)
__global__ __launch_bounds__(1024) void probe(int* __restrict__ ids, int pad, int pad_from, int busy_ticks) {
  extern __shared__ unsigned char smem[];
  const int x = blockIdx.x, y = blockIdx.y;
  unsigned xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
  if (threadIdx.x == 0) ids[y * gridDim.x + x] = (int)xcc;
  const int entry = pad == 2 ? ((x & ~7) | ((x + y) & 7)) : x;
  if (pad && (entry & 7) == 7 && (entry >> 3) >= pad_from) return;  // whole workgroup leaves before any barrier
  smem[threadIdx.x] = (unsigned char)x;  // the LDS is really used
  __syncthreads();
  // stay for busy_ticks (100 MHz) +- a quarter, bounded
  const long long t0 = wall_clock64();
  const int mine = busy_ticks + (int)(((unsigned)(x * 2654435761u + y * 40503u) >> 8) % (unsigned)(busy_ticks / 2 + 1)) - busy_ticks / 4;
  for (int i = 0; i < 100000 && wall_clock64() - t0 < mine; i++) __builtin_amdgcn_s_sleep(16);
  __syncthreads();
  if (threadIdx.x == 1 && smem[threadIdx.x] == 255 && x < 0) ids[0] = -1;  // (never: keeps the LDS traffic alive)
}

int main(int argc, char** argv) {
  const int gx = argc > 1 ? std::atoi(argv[1]) : 80, gy = argc > 2 ? std::atoi(argv[2]) : 43;
  const int lds = argc > 3 ? std::atoi(argv[3]) : 64 * 1024, busy_us = argc > 4 ? std::atoi(argv[4]) : 60;
  const int launches = argc > 5 ? std::atoi(argv[5]) : 5;
  if (gx <= 0 || gx % 8 != 0 || gy <= 0 || gx > 4096 || gy > 4096 || lds < 1024 || lds > 160 * 1024 || busy_us < 1 || busy_us > 2000 || launches < 1 || launches > 100) {
    std::printf("usage: xcd_probe [gx, a multiple of 8] [gy] [lds bytes 1024..163840] [busy us 1..2000] [launches 1..100]\n");
    return 2;
  }
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, 0));
  char pci[32] = "";
  CK(hipDeviceGetPCIBusId(pci, sizeof pci, 0));
  std::printf("device %s (%s) pci %s, grid %d x %d of 1024 threads, %d LDS bytes, ~%d us per block\n", prop.name, prop.gcnArchName, pci, gx, gy, lds, busy_us);
  if (lds > 64 * 1024) CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&probe), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  int* d_ids = nullptr;
  const size_t n = (size_t)gx * gy;
  CK(hipMalloc(&d_ids, n * sizeof(int)));
  std::vector<int> ids(n);
  int bad_total = 0;
  static const char* const kPad[] = {"no padding", "padding in fixed columns", "padding in rotated columns"};
  for (int pad = 0; pad < 3; pad++)
    for (int l = 0; l < launches; l++) {
      CK(hipMemset(d_ids, 0xff, n * sizeof(int)));
      probe<<<dim3(gx, gy), 1024, lds>>>(d_ids, pad, gx / 8 / 2, busy_us * 100);
      CK(hipGetLastError());
      CK(hipDeviceSynchronize());
      CK(hipMemcpy(ids.data(), d_ids, n * sizeof(int), hipMemcpyDeviceToHost));
      // XCD of residue r = that of block (r, 0); every block (x, y) must agree with residue x % 8; the 8 residues must be 8 XCDs
      int bad = 0, unset = 0, seen = 0;
      for (int y = 0; y < gy; y++)
        for (int x = 0; x < gx; x++) {
          const int id = ids[(size_t)y * gx + x];
          if (id < 0 || id > 7) unset++;
          else if (id != ids[x % 8]) bad++;
        }
      for (int r = 0; r < 8; r++)
        if (ids[r] >= 0 && ids[r] < 8) seen |= 1 << ids[r];
      std::printf("%-27s launch %d: residues 0..7 -> XCD %d %d %d %d %d %d %d %d   blocks off their residue's XCD: %d of %zu, without an id: %d%s\n", kPad[pad], l,
                  ids[0], ids[1], ids[2], ids[3], ids[4], ids[5], ids[6], ids[7], bad, n, unset, seen == 0xff ? "" : "   (residues share an XCD)");
      bad_total += bad + unset + (seen != 0xff);
    }
  CK(hipFree(d_ids));
  std::printf(bad_total ? "PREMISE FAILS: block (x, y) does not always run on the XCD of x %% 8\n" : "PREMISE HOLDS: block (x, y) runs on the XCD of x %% 8 in every group\n");
  return bad_total ? 1 : 0;
}
