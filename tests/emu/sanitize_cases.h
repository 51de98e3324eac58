// sanitize_cases.h — TEST INFRASTRUCTURE: the one tally of tests/emu/sanitize_driver.cpp, and the cases of the families that keep
// them next to their stepping (emu_gadget2.cpp, emu_galois.cpp, emu_extprod.cpp, emu_cmux.cpp, emu_blindrot.cpp, behind
// EMU_SANITIZE_CASES: they use what their source includes), each as one function that the driver calls.
#pragma once
#include <cstdio>

struct Tally { int checks = 0, failures = 0; };
extern Tally tally;                                        // sanitize_driver.cpp
inline void expect(bool ok, const char* what) {
  ++tally.checks;
  if (!ok) { ++tally.failures; std::printf("FAILED: %s\n", what); }
}

void gadget2_cases();
void galois_cases();
void extprod_cases();
void cmux_cases();
void blindrot_cases();
