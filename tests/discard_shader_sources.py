"""HIP C++ sources of user shaders that may discard (include/trgl.h, TRGL_SHADER_MAY_DISCARD), for the tests: registered with the
flag, trgl_fragment returns trgl_frag_out and runs for every fragment that passes the z-test, in order.  A user kind drawn with one
of them must give the frame, depths and counters of the built-in kind it restates."""
import user_shader_sources as S

# CHECKER (frag_checker_discards, kernels_raster.hip): cells = uniforms->reserved; the cell parities of the perspective-correct
# bar[0] and bar[1] differ -> discard.  (int)double as the reference's x86-64 build executes it: out of range -> INT_MIN.
CHECKER = r"""
__device__ static int checker_cvt(double d) {
    if (!(d > -2147483649.0 && d < 2147483648.0)) return -2147483647 - 1;
    return (int)d;
}
__device__ trgl_frag_out trgl_fragment(const trgl_frag_in& in) {
    const int cells = in.u->reserved;
    const int a = checker_cvt(in.bar[0] * (double)cells), c = checker_cvt(in.bar[1] * (double)cells);
    return trgl_frag_out{ ((a ^ c) & 1) != 0, in.color };
}
"""

# the same predicate written another way (parities compared; INT_MIN is even): a second kind that may discard, with the semantics
# of the first
CHECKER_B = r"""
__device__ static int checker_parity(double d) { return (d > -2147483649.0 && d < 2147483648.0) ? ((int)d & 1) : 0; }
__device__ trgl_frag_out trgl_fragment(const trgl_frag_in& in) {
    const double n = (double)in.u->reserved;
    trgl_frag_out o;
    o.discard = checker_parity(in.bar[0] * n) != checker_parity(in.bar[1] * n);
    o.bgra = in.color;
    return o;
}
"""

DISCARD_ALL = r"""
__device__ trgl_frag_out trgl_fragment(const trgl_frag_in& in) { return trgl_frag_out{ true, in.color }; }
"""

# one source for both contracts (TRGL_USER_MAY_DISCARD is 1 ahead of a source registered with the flag, else 0); each contract
# leaves a warning of its own in the compiler log
BOTH_CONTRACTS = r"""
#if TRGL_USER_MAY_DISCARD
#warning trgl-test-discarding-contract
__device__ trgl_frag_out trgl_fragment(const trgl_frag_in& in) { return trgl_frag_out{ false, in.color }; }
#else
#warning trgl-test-plain-contract
__device__ uint32_t trgl_fragment(const trgl_frag_in& in) { return in.color; }
#endif
"""

_PLAIN_SIGNATURE = "__device__ uint32_t trgl_fragment(const trgl_frag_in& in)"


def never_discarding(plain):
    """A source of the plain contract (user_shader_sources) restated for the discarding one: its colour, never discarded."""
    assert plain.count(_PLAIN_SIGNATURE) == 1
    return plain.replace(_PLAIN_SIGNATURE, "__device__ static uint32_t restated_color(const trgl_frag_in& in)") + r"""
__device__ trgl_frag_out trgl_fragment(const trgl_frag_in& in) { return trgl_frag_out{ false, restated_color(in) }; }
"""


FLAT = never_discarding(S.FLAT)
GOURAUD = never_discarding(S.GOURAUD)
PHONG = never_discarding(S.PHONG)
