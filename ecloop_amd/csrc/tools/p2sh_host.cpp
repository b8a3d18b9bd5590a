// p2sh_host.cpp — compiles hash160_p2sh of the DEVICE header hash160.h for the host with g++, so that the CPU test-suite can check
// the kernels' P2SH-P2WPKH hash without a GPU (tests/test_p2sh_host.py).  Not part of the product library.
#include "../hash160.h"
#include <stddef.h>

extern "C" {
// out[i] = hash160(0x00 0x14 || h33[i]) for n hashes of 5 h160_t words each
void ph_p2sh_many(const u32* h33, u32* out, u32 n) {
  for (u32 i = 0; i < n; ++i) hash160_p2sh(out + (size_t)i * 5, h33 + (size_t)i * 5);
}
}
