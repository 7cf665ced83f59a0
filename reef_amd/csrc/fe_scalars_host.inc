// The scalar checks of the conversion layer's host side (fe_host.inc includes this first): a caller's field element is below the
// modulus, and comes in as internal form or as a canonical integer.  Plain host arithmetic over field.h: no HIP, no state, so a host
// program can compile it alone (host/ipa_batch_selftest.cpp).  Needs reef_status, REEF_TRY and set_error (common.h).
#pragma once                     // keygen_engine.inc (inside engine.inc) takes fe_valid before fe_host.inc includes this
namespace reef {

static bool fe_valid(const reef_fe *x, int field) {              // canonical: below the modulus
    fe256 p;
    memcpy(&p, x, sizeof p);
    const u32 *m = field == 0 ? FC<0>::MOD : FC<1>::MOD;
    fe v = fe_unpack(p);
    for (int i = 8; i >= 0; --i)
        if (v.l[i] != m[i]) return v.l[i] < m[i];
    return false;
}
template <int F> static fe fe_import(const reef_fe *x, bool is_mont) {
    fe256 p;
    memcpy(&p, x, sizeof p);
    return fe_canon<F>(fe_from_caller<F>(p, is_mont));
}
// `count` elements below the modulus, in the caller's form -> internal form (Out = fe) or canonical integers (Out = fe256)
template <int F, class Out>
static reef_status fe_import_all(const reef_fe *x, size_t count, bool is_mont, const char *name, const char *what, Out *out) {
    for (size_t i = 0; i < count; ++i) {
        if (!fe_valid(x + i, F)) { set_error("%s: %s[%zu] is not below the modulus", name, what, i); return REEF_ERR_ARG; }
        const fe v = fe_import<F>(x + i, is_mont);
        if constexpr (std::is_same<Out, fe>::value) out[i] = v;
        else out[i] = fe_to_integer<F>(v);
    }
    return REEF_OK;
}
// the challenge of a call: canonical when given as an integer; nonzero: an IPA fold, which needs r^-1
template <int F> static reef_status fe_challenge(const reef_fe *r, bool is_mont, const char *name, fe &out, bool nonzero = false) {
    if (!r) { set_error("null argument"); return REEF_ERR_ARG; }
    if (!fe_valid(r, F)) { set_error("%s: r is not below the modulus", name); return REEF_ERR_ARG; }
    out = fe_import<F>(r, is_mont);
    if (nonzero && fe_is_literal_zero(fe_canon<F>(out))) { set_error("%s: r is zero (it has no inverse)", name); return REEF_ERR_ARG; }
    return REEF_OK;
}

}  // namespace reef
