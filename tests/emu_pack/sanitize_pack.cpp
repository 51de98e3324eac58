// sanitize_pack.cpp — TEST INFRASTRUCTURE: the pack / trace step stepping and the LWE embedding's under AddressSanitizer + UBSan,
// as a stand-alone program beside sanitize_driver, sanitize_galoisks and sanitize_lwe: the cases stand next to the stepping
// (emu_pack.cpp, behind EMU_SANITIZE_CASES) and compare it with the steppings of the explicit route (tests/emu/emu_cmux.cpp,
// tests/emu_galoisks/emu_galoisks.cpp), which are compiled in.  make -C tests/emu_pack sanitize; tests/test_pack_emu.py runs it.
#include "../emu/sanitize_cases.h"

Tally tally;
void pack_cases();

int main() {
  pack_cases();
  std::printf("pack: %d checks\n", tally.checks);
  std::printf("sanitize_pack: %d checks, %d failures\n", tally.checks, tally.failures);
  return tally.failures ? 1 : 0;
}
