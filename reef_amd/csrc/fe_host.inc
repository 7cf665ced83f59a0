// Host side of the conversion layer (fe_vec.h): scalars in the caller's form on their way into a row's state machine, the eq table
// over a point, and the check of a borrowed key.  Included after engine.inc and before the rows that sit on a resident context
// (nifs_engine.inc, ipa_engine.inc, spartan_engine.inc, open_engine.inc, hyrax_engine.inc).
#include "fe_scalars_host.inc"   // fe_valid, fe_import, fe_import_all, fe_challenge: the part that needs no device
namespace reef {

// eq(p) over 2^ell entries into dst (internal form) on `st`; the 2 ell factors go through `pts`.  Waits for the stream.
template <int F> static reef_status fe_eq_table(hipStream_t st, DevBuf &pts, const fe *p, u32 ell, fe256 *dst) {
    std::vector<fe256> f(2 * std::max<u32>(ell, 1));
    for (u32 j = 0; j < ell; ++j) {
        f[2 * j] = fe_to_table<F>(fe_sub<F, 2>(fe_one<F>(), p[j]));
        f[2 * j + 1] = fe_to_table<F>(p[j]);
    }
    REEF_TRY(pts.ensure(f.size() * sizeof(fe256)));
    REEF_HIP_TRY(hipMemcpyAsync(pts.p, f.data(), f.size() * sizeof(fe256), hipMemcpyHostToDevice, st));
    const size_t n = (size_t)1 << ell;
    hipLaunchKernelGGL(k_sp_eq<F>, dim3(ceil_div(n, 256)), dim3(256), 0, st, (const fe256 *)pts.p, ell, (u32)n, dst);
    REEF_HIP_TRY(hipGetLastError());
    REEF_HIP_TRY(hipStreamSynchronize(st));                    // f goes out of scope
    return REEF_OK;
}

// The MSM key a row borrows lives on the row's device (REEF_ERR_ARG in the words of the call `name` on the `owner` ctx otherwise);
// *n: the points it holds, for the row's own check of the length.  Both are read under the key ctx's lock.
template <int C> static reef_status key_matches(Ctx<C> *key, int device, const char *name, const char *owner, size_t *n) {
    int key_dev = 0;
    {
        std::lock_guard<std::mutex> kl(key->mu);
        key_dev = key->key->device;
        *n = key->key->n;
    }
    if (key_dev != device) { set_error("%s: the key lives on device %d, the %s ctx on device %d", name, key_dev, owner, device); return REEF_ERR_ARG; }
    return REEF_OK;
}

}  // namespace reef
