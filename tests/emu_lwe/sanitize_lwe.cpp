// sanitize_lwe.cpp — TEST INFRASTRUCTURE: the LWE kernels' stepping under AddressSanitizer + UBSan, as a stand-alone program
// beside sanitize_driver and sanitize_galoisks: the cases stand next to the stepping (emu_lwe.cpp, behind EMU_SANITIZE_CASES).
// make -C tests/emu_lwe sanitize; tests/test_lwe_emu.py runs it.
#include "../emu/sanitize_cases.h"

Tally tally;
void lwe_cases();

int main() {
  lwe_cases();
  std::printf("lwe: %d checks\n", tally.checks);
  std::printf("sanitize_lwe: %d checks, %d failures\n", tally.checks, tally.failures);
  return tally.failures ? 1 : 0;
}
