// Vesta instantiation of the MSM engine (coordinates in Fq, scalars in Fp).
#define REEF_CURVE 1
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
namespace reef {
const CurveVTable *vesta_vtable() {
    static const CurveVTable vt = make_vtable<1>();
    return &vt;
}
const NifsVTable *vesta_nifs_vtable() {
    static const NifsVTable vt = make_nifs_vtable<1>();
    return &vt;
}
const SpartanVTable *vesta_spartan_vtable() {
    static const SpartanVTable vt = make_spartan_vtable<1>();
    return &vt;
}
const OpenVTable *vesta_open_vtable() {
    static const OpenVTable vt = make_open_vtable<1>();
    return &vt;
}
const HyraxVTable *vesta_hyrax_vtable() {
    static const HyraxVTable vt = make_hyrax_vtable<1>();
    return &vt;
}
const HyraxBatchVTable *vesta_hyrax_batch_vtable() {
    static const HyraxBatchVTable vt = make_hyrax_batch_vtable<1>();
    return &vt;
}
const HyraxVkVTable *vesta_hyrax_vk_vtable() {
    static const HyraxVkVTable vt = make_hyrax_vk_vtable<1>();
    return &vt;
}
const IpaCheckVTable *vesta_ipa_check_vtable() {
    static const IpaCheckVTable vt = make_ipa_check_vtable<1>();
    return &vt;
}
const MerkleVTable *vesta_merkle_vtable() {
    static const MerkleVTable vt = make_merkle_vtable<1>();
    return &vt;
}
}
