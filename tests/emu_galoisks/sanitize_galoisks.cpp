// sanitize_galoisks.cpp — TEST INFRASTRUCTURE: the automorphism key-switch stepping under AddressSanitizer + UBSan, as a
// stand-alone program beside sanitize_driver (whose printed family lines tests/test_emu.py pins): the cases stand next to the
// stepping (emu_galoisks.cpp, behind EMU_SANITIZE_CASES) and compare it with the steppings of the explicit route
// (tests/emu/emu_galois.cpp, emu_gadget2.cpp), which are compiled in.  make -C tests/emu_galoisks sanitize; tests/test_galoisks_emu.py runs it.
#include "../emu/sanitize_cases.h"

Tally tally;
void galoisks_cases();

int main() {
  galoisks_cases();
  std::printf("galoisks: %d checks\n", tally.checks);
  std::printf("sanitize_galoisks: %d checks, %d failures\n", tally.checks, tally.failures);
  return tally.failures ? 1 : 0;
}
