// eth_host.cpp — compiles eth_address of the DEVICE header keccak.h for the host with g++, so that the CPU test-suite can check the
// kernels' Keccak-256 without a GPU (tests/test_eth_host.py).  Not part of the product library.
#include "../keccak.h"
#include <stddef.h>

extern "C" {
// out[i] = Ethereum address (5 h160_t words) of the coordinates xw[i], yw[i] (8 canonical little-endian words each)
void eh_eth_many(const u32* xw, const u32* yw, u32* out, u32 n) {
  for (u32 i = 0; i < n; ++i) eth_address(out + (size_t)i * 5, xw + (size_t)i * 8, yw + (size_t)i * 8);
}
}
