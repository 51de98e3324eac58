// sanitize_lwe_mfma.cpp — TEST INFRASTRUCTURE: the stepping of the matrix-core key switch under AddressSanitizer + UBSan, as a
// stand-alone program beside sanitize_driver, sanitize_galoisks and sanitize_lwe: the cases stand next to the stepping
// (emu_lwe_mfma.cpp, behind EMU_SANITIZE_CASES).  make -C tests/emu_lwe_mfma sanitize; tests/test_lwe_mfma_emu.py runs it.
#include "../emu/sanitize_cases.h"

Tally tally;
void lwe_mfma_cases();

int main() {
  lwe_mfma_cases();
  std::printf("sanitize_lwe_mfma: %d checks, %d failures\n", tally.checks, tally.failures);
  return tally.failures ? 1 : 0;
}
