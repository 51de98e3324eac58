// cmux_core.h — the per-word code of the monomial product X^e * a and of the CMux rotation step, free of HIP: the kernels of
// kernels_cmux.hip and their CPU stepping (tests/emu_cmux) are compiled from it.  include/tinyntt.h has the definition.
#pragma once
#include "fused_core.h"

namespace tn {

// Where word t of rot_e(x) comes from: v = (t - e) mod 2n is any value congruent to it with bit log2 n intact (the callers add
// a register's offset below n to (thread - e) & (2n - 1): below 3n, bit log2 n of the sum is that of the sum mod 2n).
// The index is MASKED to the row, so no exponent addresses a word outside it.
TN_HD u32 monomial_index(u32 v, u32 logn) { return v & ((1u << logn) - 1u); }
TN_HD bool monomial_negated(u32 v, u32 logn) { return ((v >> logn) & 1u) != 0; }

// a canonical residue with the wrap's sign applied: a zero stays 0, never q
template <typename E>
TN_HD E monomial_signed(E x, bool neg, E q) { return neg ? (x ? (E)(q - x) : (E)0) : x; }

// (s - o) mod q for canonical s and o (s + (q - o) < 2q fits the word: q < 2^31 / 2^63)
template <typename E>
TN_HD E sub_canonical(E s, E o, E q) { return s >= o ? (E)(s - o) : (E)(s + (E)(q - o)); }

// One word of (X^e - 1) * a under the plan's policy: `rot` is the word of the row that the rotation brings here, `own` the word
// that is here; any word values.  What tn_monomial_mul_dev writes with TN_MONOMIAL_MINUS_ONE, so the digits cut from it are
// the explicit route's.
template <typename E, typename Pol>
TN_HD E cmux_word(E own, E rot, bool neg, const Arith<E>& ar) {
  const E o = gadget_canon<E, Pol>(own, ar);
  const E s = monomial_signed<E>(gadget_canon<E, Pol>(rot, ar), neg, ar.q);
  return sub_canonical<E>(s, o, ar.q);
}

// The add-in at the store: (a mod q + x) mod q for a canonical x (an inverse transform's output) and any word a
template <typename E, typename Pol>
TN_HD E cmux_add_in(E x, E a, const Arith<E>& ar) { return csub((E)(x + gadget_canon<E, Pol>(a, ar)), ar.q); }

// One word of tn_monomial_mul_dev on any plan: the canonicalisation is the canonical policy's (mul_tw by one: x mod q for any
// word, as gadget_decompose_kernel and pointwise_kernel take their inputs)
template <typename E>
TN_HD E monomial_word(E own, E rot, bool neg, bool minus_one, const Arith<E>& ar) {
  const E s = monomial_signed<E>(mul_tw(rot, ar.one, ar.q), neg, ar.q);
  return minus_one ? sub_canonical<E>(s, mul_tw(own, ar.one, ar.q), ar.q) : s;
}

}  // namespace tn
