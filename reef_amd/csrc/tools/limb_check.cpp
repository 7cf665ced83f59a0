// Host build of the loop-form key-table record (ec.h: affine_limbs) with bound tracking (REEF_BOUNDS): what k_limb_tables
// stores for a packed table entry, what k_accum0 reads back from it, and both forms of the accumulation loop side by side.
// TEST HARNESS ONLY (tests/test_limb_tables_host.py) -- the product never links this.
//   g++ -O2 -std=c++17 -DREEF_BOUNDS -shared -fPIC limb_check.cpp -o libreef_limbcheck.so
#include <string.h>

#include "../ec.h"

using namespace reef;

// the words one entry loads from a record, as load_limbs_entry (msm_kernels.inc) picks them
static limbs_entry entry_of(const affine_limbs &rec, bool neg) {
    limbs_entry e;
    for (int i = 0; i < 12; ++i) e.head[i] = rec.w[i];
    for (int i = 0; i < 8; ++i) e.ysel[i] = rec.w[(neg ? LIMBS_NEG_Y : LIMBS_Y) + i];
    return e;
}

template <int C> static void record(const affine256 *packed, u32 *rec, u32 *x, u32 *y, u32 *ny) {
    const affine_limbs r = affine_limbs_from_table<C>(*packed);
    memcpy(rec, r.w, sizeof r.w);
    const fe fx = fe_from_table(packed->x), fy = fe_from_table(packed->y), fn = fe_neg<C, 2>(fy);   // what the loop computes from the packed entry
    memcpy(x, fx.l, 36); memcpy(y, fy.l, 36); memcpy(ny, fn.l, 36);
}

template <int C> static int entry(const u32 *rec, int neg, u32 *x, u32 *y) {
    affine_limbs r;
    memcpy(r.w, rec, sizeof r.w);
    bool inf;
    const affine p = affine_from_limbs(entry_of(r, neg != 0), neg != 0, &inf);
    memcpy(x, p.x.l, 36); memcpy(y, p.y.l, 36);
    return inf ? 1 : 0;
}

// acc = sum_i (+/-) pts[i] over packed table entries, by the loop on the packed tables and by the loop on the records: the
// accumulators must agree limb for limb after every entry (-> 1), and REEF_BOUNDS aborts where a formula's bound is missed.
template <int C> static int chains(const affine256 *pts, const uint8_t *neg, size_t n, u32 *out) {
    xyzz a = xyzz_identity(), b = xyzz_identity();
    bool empty = true;
    int same = 1;
    for (size_t i = 0; i < n; ++i) {
        affine pt = affine_from_table(pts[i]);
        pt.y = fe_select(neg[i] && !affine_is_inf(pt), fe_neg<C, 2>(pt.y), pt.y);
        a = xyzz_madd_flag<C>(a, empty, pt);
        const affine_limbs rec = affine_limbs_from_table<C>(pts[i]);
        bool inf;
        const affine q = affine_from_limbs(entry_of(rec, neg[i] != 0), neg[i] != 0, &inf);
        b = xyzz_madd_flags<C>(b, empty, q, inf);
        empty = false;
        const xyzz_mem ma = xyzz_to_mem(a), mb = xyzz_to_mem(b);
        if (memcmp(ma.w, mb.w, sizeof ma.w) != 0) same = 0;
        a = xyzz_from_mem(ma); b = xyzz_from_mem(mb);
    }
    const xyzz_mem m = xyzz_to_mem(b);
    memcpy(out, m.w, sizeof m.w);
    return same;
}

extern "C" {
// packed: 16 words (x, y of a table entry) -> rec: the 32 words of its record; x, y, ny: 9 limbs each of fe_from_table(x), fe_from_table(y), fe_neg<F, 2>(y)
void limb_record(int f, const void *packed, void *rec, void *x, void *y, void *ny) {
    if (f == 0) record<0>((const affine256 *)packed, (u32 *)rec, (u32 *)x, (u32 *)y, (u32 *)ny);
    else record<1>((const affine256 *)packed, (u32 *)rec, (u32 *)x, (u32 *)y, (u32 *)ny);
}
// rec -> the operand the loop gets for a digit of this sign (9 limbs each); returns the identity flag
int limb_entry(int f, const void *rec, int neg, void *x, void *y) {
    return f == 0 ? entry<0>((const u32 *)rec, neg, (u32 *)x, (u32 *)y) : entry<1>((const u32 *)rec, neg, (u32 *)x, (u32 *)y);
}
// ABI point -> packed table entry (16 words)
void limb_to_table(int f, const void *abi, void *packed) {
    const affine256 *p = (const affine256 *)abi;
    affine256 t = f == 0 ? affine_to_table<0>(affine_from_abi<0>(*p)) : affine_to_table<1>(affine_from_abi<1>(*p));
    memcpy(packed, &t, sizeof t);
}
int limb_chains(int f, const void *pts, const void *neg, size_t n, void *out) {
    return f == 0 ? chains<0>((const affine256 *)pts, (const uint8_t *)neg, n, (u32 *)out) : chains<1>((const affine256 *)pts, (const uint8_t *)neg, n, (u32 *)out);
}
}
