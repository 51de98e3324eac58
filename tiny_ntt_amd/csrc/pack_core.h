// pack_core.h — the per-word code of one level of the LWE -> RLWE packing tree and of a trace step
// (polydot_pack_kernel, kernels_pack.hip), free of HIP: the kernel and its CPU stepping (tests/emu_pack) are
// compiled from it.  include/tinyntt.h has the definition.  With t = X^rot * od: s = ev + t, d = ev - t, every input word taken
// mod q; sigma_g(d) goes through the transpose image (galois_dst), s is added at the stores.
#pragma once
#include "galois_core.h"
#include "cmux_core.h"

namespace tn {

// One word of t = X^rot * od as a canonical residue: `rot` is the word the rotation brings here (monomial_index), any value;
// what tn_monomial_mul_dev writes.
template <typename E, typename Pol>
TN_HD E pack_rotated_word(E rot, bool neg, const Arith<E>& ar) { return monomial_signed<E>(gadget_canon<E, Pol>(rot, ar), neg, ar.q); }

// One word of d = ev - t and of s = ev + t: ev any word, t canonical.  One conditional step each.
template <typename E, typename Pol>
TN_HD E pack_diff_word(E ev, E t, const Arith<E>& ar) { return sub_canonical<E>(gadget_canon<E, Pol>(ev, ar), t, ar.q); }
template <typename E, typename Pol>
TN_HD E pack_sum_word(E ev, E t, const Arith<E>& ar) { return csub((E)(gadget_canon<E, Pol>(ev, ar) + t), ar.q); }

// A canonical word of d on its way to the image under sigma_g: the wrap's sign; a zero stays 0 (galois_scatter_word without
// its canonicalisation, which pack_diff_word has done)
template <typename E> TN_HD E pack_scatter_word(E d, bool negate, E q) { return negate ? galois_neg(d, q) : d; }

// The add-in at a store: (x + s) mod q for canonical x (an inverse transform's output, or a sum of two) and canonical s
template <typename E> TN_HD E pack_add_in(E x, E s, E q) { return csub((E)(x + s), q); }

}  // namespace tn
