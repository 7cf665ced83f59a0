// Pallas instantiation of the MSM engine (coordinates in Fp, scalars in Fq).
#define REEF_CURVE 0
#include "msm_kernels.inc"
#include "fe_vec.h"
#include "sumcheck_kernels.inc"
#include "mle_kernels.inc"
#include "merkle_kernels.inc"
#include "keygen_kernels.inc"
#include "decompress_kernels.inc"
#include "nifs_kernels.inc"
#include "spartan_kernels.inc"
#include "open_kernels.inc"
#include "hyrax_kernels.inc"
#include "hyrax_batch_kernels.inc"
#include "ipa_check_kernels.inc"
#include "doc_kernels.inc"
#include "engine.inc"
#include "fe_host.inc"
#include "nifs_engine.inc"
#include "proof_order.h"
#include "ipa_engine.inc"
#include "ipa_check_engine.inc"
#include "spartan_engine.inc"
#include "open_engine.inc"
#include "hyrax_engine.inc"
#include "hyrax_vk_engine.inc"
#include "hyrax_batch_engine.inc"
#include "merkle_resident_engine.inc"
#include "doc_engine.inc"      // once: both curves' tables point at it
namespace reef {
const CurveVTable *pallas_vtable() {
    static const CurveVTable vt = make_vtable<0>();
    return &vt;
}
const NifsVTable *pallas_nifs_vtable() {
    static const NifsVTable vt = make_nifs_vtable<0>();
    return &vt;
}
const SpartanVTable *pallas_spartan_vtable() {
    static const SpartanVTable vt = make_spartan_vtable<0>();
    return &vt;
}
const OpenVTable *pallas_open_vtable() {
    static const OpenVTable vt = make_open_vtable<0>();
    return &vt;
}
const HyraxVTable *pallas_hyrax_vtable() {
    static const HyraxVTable vt = make_hyrax_vtable<0>();
    return &vt;
}
const HyraxBatchVTable *pallas_hyrax_batch_vtable() {
    static const HyraxBatchVTable vt = make_hyrax_batch_vtable<0>();
    return &vt;
}
const HyraxVkVTable *pallas_hyrax_vk_vtable() {
    static const HyraxVkVTable vt = make_hyrax_vk_vtable<0>();
    return &vt;
}
const IpaCheckVTable *pallas_ipa_check_vtable() {
    static const IpaCheckVTable vt = make_ipa_check_vtable<0>();
    return &vt;
}
const MerkleVTable *pallas_merkle_vtable() {
    static const MerkleVTable vt = make_merkle_vtable<0>();
    return &vt;
}
}
