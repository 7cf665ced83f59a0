// Row N1 of SURVEY.md 8f: derivation of the commitment key on the GPU.
//
// Reef derives its generators on every --prove and --verify (PublicParams::setup, src/backend/framework.rs:297-303;
// SpartanSNARK::setup and HyraxPC::setup, src/backend/commitment.rs:146-149,176-180) through nova-snark's
// CommitmentGens::new(label, n) -> from_label [R]: SHAKE256(label) squeezed into n 32-byte strings, each hashed to the
// curve with pasta_curves' hash_to_curve("from_uniform_bytes") [R], i.e. the hash_to_curve of RFC 9380 for
// <curve>_XMD:BLAKE2b_SSWU_RO_.  The XOF is sequential and runs on the host (keccak.h, 4 MiB for 2^17 generators); this
// file is the per-generator part, one thread each:
//   hash_to_field   expand_message_xmd over BLAKE2b-512 (RFC 9380 5.3.1) -> two elements of the base field (5.2)
//   map_to_curve    simplified SWU on E': y^2 = x^3 + a x + b (appendix F.2 straight-line form; square roots by Tonelli-Shanks
//                   on the 2^32 two-adicity of the Pasta fields), then the 3-isogeny to y^2 = x^3 + 5 evaluated projectively
//   sum             the two images added (xyzz_add), normalised afterwards by k_xyzz_normalize
// Everything pasta_curves fixes and this repository cannot confirm -- a, b, Z, the 13 isogeny coefficients, the domain
// separation string, the byte order of hash_to_field -- is DATA of the call (reef_keygen_params).
//
// Included by kernels_<curve>.hip after fe_vec.h; C = curve, coordinates in field C.
namespace reef {

// ---- BLAKE2b-512, unkeyed (RFC 7693) ----
__device__ __forceinline__ u64 rotr64(u64 x, int r) { return (x >> r) | (x << (64 - r)); }
__device__ void blake2b_compress(u64 (&h)[8], const unsigned char *block, u64 t, bool last) {
    const u64 IV[8] = {0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL, 0xa54ff53a5f1d36f1ULL,
                       0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL, 0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};
    const unsigned char SIGMA[12][16] = {
        {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
        {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
        {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
        {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
        {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0},
        {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3}};
    u64 m[16], v[16];
    for (int i = 0; i < 16; ++i) {
        u64 w = 0;
        for (int k = 7; k >= 0; --k) w = (w << 8) | block[8 * i + k];
        m[i] = w;
    }
    for (int i = 0; i < 8; ++i) { v[i] = h[i]; v[8 + i] = IV[i]; }
    v[12] ^= t;                       // messages here are far below 2^64 bytes: the high counter word stays zero
    if (last) v[14] = ~v[14];
    for (int r = 0; r < 12; ++r) {
        const unsigned char *s = SIGMA[r];
#define REEF_B2B_G(a, b, c, d, x, y)                                   \
        v[a] = v[a] + v[b] + (x); v[d] = rotr64(v[d] ^ v[a], 32);     \
        v[c] = v[c] + v[d];       v[b] = rotr64(v[b] ^ v[c], 24);     \
        v[a] = v[a] + v[b] + (y); v[d] = rotr64(v[d] ^ v[a], 16);     \
        v[c] = v[c] + v[d];       v[b] = rotr64(v[b] ^ v[c], 63);
        REEF_B2B_G(0, 4, 8, 12, m[s[0]], m[s[1]])
        REEF_B2B_G(1, 5, 9, 13, m[s[2]], m[s[3]])
        REEF_B2B_G(2, 6, 10, 14, m[s[4]], m[s[5]])
        REEF_B2B_G(3, 7, 11, 15, m[s[6]], m[s[7]])
        REEF_B2B_G(0, 5, 10, 15, m[s[8]], m[s[9]])
        REEF_B2B_G(1, 6, 11, 12, m[s[10]], m[s[11]])
        REEF_B2B_G(2, 7, 8, 13, m[s[12]], m[s[13]])
        REEF_B2B_G(3, 4, 9, 14, m[s[14]], m[s[15]])
#undef REEF_B2B_G
    }
    for (int i = 0; i < 8; ++i) h[i] ^= v[i] ^ v[8 + i];
}
// out[64] = BLAKE2b-512(in[0..len))
__device__ void blake2b_512(const unsigned char *in, u32 len, unsigned char *out) {
    u64 h[8] = {0x6a09e667f3bcc908ULL ^ 0x01010040ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL, 0xa54ff53a5f1d36f1ULL,
                0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL, 0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};
    unsigned char block[128];
    u32 off = 0;
    while (len - off > 128) {
        for (int k = 0; k < 128; ++k) block[k] = in[off + k];
        off += 128;
        blake2b_compress(h, block, off, false);
    }
    const u32 rem = len - off;            // 0..128 (0 only for an empty message)
    for (u32 k = 0; k < 128; ++k) block[k] = k < rem ? in[off + k] : 0;
    blake2b_compress(h, block, len, true);
    for (int i = 0; i < 8; ++i)
        for (int k = 0; k < 8; ++k) out[8 * i + k] = (unsigned char)(h[i] >> (8 * k));
}

// ---- field helpers of the maps ----
template <int F> __device__ __forceinline__ bool fe_equal(const fe &a, const fe &b) { return fe_is_zero<F>(fe_sub<F, 4>(a, b)); }   // a, b < 4
template <int F> __device__ __forceinline__ u32 fe_sgn0(const fe &x) { return fe_to_integer<F>(x).w[0] & 1u; }                      // parity of the canonical integer
// 64 bytes (OS2IP big-endian, or little-endian) mod M -> internal form
template <int F> __device__ fe fe_from_64_bytes(const unsigned char *s, bool little_endian) {
    fe acc = fe_zero();
    REEF_SET_BOUND(acc, 1.0);
    const fe c64 = fe_const<F>(FC<F>::C_2_64, 1.0);
    for (int j = 0; j < 8; ++j) {                       // most significant 64-bit word first
        u64 w = 0;
        for (int k = 0; k < 8; ++k) {
            const int pos = little_endian ? 63 - (8 * j + k) : 8 * j + k;
            w = (w << 8) | s[pos];
        }
        fe256 wv;
        wv.w[0] = (u32)w; wv.w[1] = (u32)(w >> 32);
        for (int k = 2; k < 8; ++k) wv.w[k] = 0;
        acc = fe_add<F>(fe_mul<F>(acc, c64), fe_from_integer<F>(wv));     // < 4
    }
    return fe_mul<F>(acc, fe_one<F>());                 // < 2
}
// x^e for the 222-bit exponent (T - 1)/2 of Tonelli-Shanks
template <int F> __device__ fe fe_pow_ts(const fe &x) {
    fe acc = fe_one<F>();
    for (int i = 221; i >= 0; --i) {
        acc = fe_sqr<F>(acc);
        if ((FC<F>::TS_EXP[i >> 5] >> (i & 31)) & 1u) acc = fe_mul<F>(acc, x);
    }
    return acc;
}
// square root (Tonelli-Shanks, M - 1 = 2^32 * T): true and a root, or false for a non-residue.  x < 2.
template <int F> __device__ bool fe_sqrt(const fe &x, fe &root) {
    root = fe_zero();
    REEF_SET_BOUND(root, 1.0);
    if (fe_is_zero<F>(x)) return true;
    const fe one = fe_one<F>();
    const fe w = fe_pow_ts<F>(x);
    fe r = fe_mul<F>(x, w), t = fe_mul<F>(r, w), c = fe_const<F>(FC<F>::TS_ROOT, 1.0);
    u32 m = 32;
    for (int guard = 0; guard < 40; ++guard) {
        if (fe_equal<F>(t, one)) { root = r; return true; }
        u32 i = 0;
        fe t2 = t;
        do { t2 = fe_sqr<F>(t2); ++i; } while (i < m && !fe_equal<F>(t2, one));
        if (i >= m) return false;                       // t has order 2^m: x is not a square
        fe b = c;
        for (u32 k = 0; k + i + 1 < m; ++k) b = fe_sqr<F>(b);
        r = fe_mul<F>(r, b);
        c = fe_sqr<F>(b);
        t = fe_mul<F>(t, c);
        m = i;
    }
    return false;
}

struct KeygenDev {
    const fe256 *consts;         // internal form: a, b, z, iso[13]
    const unsigned char *dst;    // domain separation string
    u32 dst_len;
    u32 little_endian;
};

// simplified SWU (RFC 9380 F.2) followed by the isogeny: u -> a point of y^2 = x^3 + 5 in XYZZ form
template <int C> __device__ xyzz sswu_iso(const fe &u, const KeygenDev &kd) {
    const fe A = fe_from_table(load_fe256(kd.consts + 0)), B = fe_from_table(load_fe256(kd.consts + 1)), Z = fe_from_table(load_fe256(kd.consts + 2));
    const fe one = fe_one<C>();
    const fe tv1 = fe_mul<C>(Z, fe_sqr<C>(u));
    const fe tv2 = fe_mul<C>(fe_add<C>(fe_sqr<C>(tv1), tv1), one);                 // < 2
    const fe tv3 = fe_mul<C>(B, fe_add<C>(tv2, one));
    const bool z2 = fe_is_zero<C>(tv2);
    const fe tv4 = fe_mul<C>(A, fe_select(z2, Z, fe_neg<C, 2>(tv2)));
    fe tv6 = fe_sqr<C>(tv4);
    const fe tv4sq = tv6;
    fe gx = fe_mul<C>(fe_add<C>(fe_sqr<C>(tv3), fe_mul<C>(A, tv6)), tv3);           // (tv3^2 + A tv4^2) tv3
    tv6 = fe_mul<C>(tv6, tv4);
    gx = fe_mul<C>(fe_add<C>(gx, fe_mul<C>(B, tv6)), one);                          // numerator of g(x1); denominator tv6 = tv4^3
    const fe inv6 = fe_inv<C>(tv6);                                                 // the map's ONE inversion: 1 / tv4 = tv4^2 / tv4^3 below
    const fe ratio = fe_mul<C>(gx, inv6);
    fe y1;
    const bool sq = fe_sqrt<C>(ratio, y1);
    fe x = tv3, y = y1;
    if (!sq) {
        fe y2;
        (void)fe_sqrt<C>(fe_mul<C>(Z, ratio), y2);                                  // Z * g(x1) is a square when g(x1) is not
        x = fe_mul<C>(tv1, tv3);
        y = fe_mul<C>(fe_mul<C>(tv1, u), y2);
    }
    if (fe_sgn0<C>(u) != fe_sgn0<C>(y)) y = fe_mul<C>(fe_neg<C, 2>(y), one);
    x = fe_mul<C>(x, fe_mul<C>(inv6, tv4sq));
    // isogeny, projectively: x' = xn/xd, y' = y * yn/yd with Z = xd*yd: X = xn*xd*yd^2, Y = y*yn*xd^3*yd^2, ZZ = Z^2, ZZZ = Z^3
    const fe256 *k = kd.consts + 3;
    auto K = [&](int i) { return fe_from_table(load_fe256(k + i)); };
    fe xn = fe_add<C>(fe_mul<C>(K(0), x), K(1));
    xn = fe_add<C>(fe_mul<C>(xn, x), K(2));
    xn = fe_mul<C>(fe_add<C>(fe_mul<C>(xn, x), K(3)), one);
    fe xd = fe_mul<C>(fe_add<C>(x, K(4)), x);
    xd = fe_mul<C>(fe_add<C>(xd, K(5)), one);
    fe yn = fe_add<C>(fe_mul<C>(K(6), x), K(7));
    yn = fe_add<C>(fe_mul<C>(yn, x), K(8));
    yn = fe_mul<C>(fe_add<C>(fe_mul<C>(yn, x), K(9)), one);
    fe yd = fe_mul<C>(fe_add<C>(x, K(10)), x);
    yd = fe_mul<C>(fe_add<C>(yd, K(11)), x);
    yd = fe_mul<C>(fe_add<C>(yd, K(12)), one);
    const fe zc = fe_mul<C>(xd, yd), yd2 = fe_sqr<C>(yd);
    xyzz r;
    r.zz = fe_sqr<C>(zc);
    r.zzz = fe_mul<C>(r.zz, zc);
    r.x = fe_mul<C>(fe_mul<C>(xn, xd), yd2);
    r.y = fe_mul<C>(fe_mul<C>(fe_mul<C>(y, yn), fe_mul<C>(fe_sqr<C>(xd), xd)), yd2);
    return r;                                                                       // a kernel point has xd = yd = 0: the identity
}

// TWO LANES PER GENERATOR: chunk (32 bytes of the XOF) -> XYZZ point.  The kernel is a latency chain (two maps to the curve of
// ~900 dependent field products each), and the two maps of a generator are independent: lanes 2g and 2g + 1 both expand the
// message (byte work, cheap beside the maps), map u0 / u1, and lane 2g adds the two images.
template <int C>
__global__ void __launch_bounds__(64) k_hash_to_curve(const unsigned char *__restrict__ chunks, u32 n, KeygenDev kd, xyzz_mem *__restrict__ out) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 i = t >> 1, which = t & 1u;
    const bool live = i < n;
    xyzz q = xyzz_identity();
    if (live) {
        // expand_message_xmd(msg, DST, 128): b0 = H(Z_pad || msg || I2OSP(128, 2) || 0 || DST'), b1 = H(b0 || 1 || DST'), b2 = H((b0 ^ b1) || 2 || DST')
        unsigned char buf[128 + 32 + 3 + 256], b0[64], uniform[128];
        const u32 dl = kd.dst_len;
        u32 len = 0;
        for (int k = 0; k < 128; ++k) buf[len++] = 0;
        for (int k = 0; k < 32; ++k) buf[len++] = chunks[(size_t)i * 32 + k];
        buf[len++] = 0; buf[len++] = 128; buf[len++] = 0;
        for (u32 k = 0; k < dl; ++k) buf[len++] = kd.dst[k];
        buf[len++] = (unsigned char)dl;
        blake2b_512(buf, len, b0);
        for (int round = 1; round <= 2; ++round) {
            len = 0;
            for (int k = 0; k < 64; ++k) buf[len++] = round == 1 ? b0[k] : (unsigned char)(b0[k] ^ uniform[k]);
            buf[len++] = (unsigned char)round;
            for (u32 k = 0; k < dl; ++k) buf[len++] = kd.dst[k];
            buf[len++] = (unsigned char)dl;
            blake2b_512(buf, len, uniform + 64 * (round - 1));
        }
        const fe u = fe_from_64_bytes<C>(uniform + 64 * which, kd.little_endian != 0);
        q = sswu_iso<C>(u, kd);
    }
    const xyzz other = shfl_xyzz(q, (int)((threadIdx.x & 63u) ^ 1u));      // every lane of the wave takes part
    if (live && which == 0) store_xyzz(out + i, xyzz_add<C>(q, other));
}

}  // namespace reef
