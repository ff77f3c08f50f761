// ecdsa_wide_curves.hpp — the six 384- and 512-bit prime-field curves of
// include/lcb_ecdsa_wide_gpu.h as data: the library's own restatement of
// these public domain parameters (SEC 2, RFC 5639, RFC 7836 /
// GOST R 34.10-2012), under the names of the reference's table
// (ecdsa.h:96-739).  All have cofactor 1.  tests/test_ecdsa_wide_model.py
// compares them with what the reference's loaded curves export
// (tests/golden/ecdsa_wide.json).
#pragma once
#include <stdint.h>

namespace lcbec {

struct WideCurveText {
    const char* name;
    uint32_t algo;       // kAlgoEcdsa / kAlgoGost
    uint32_t bytes;      // B: 48 or 64
    const char* num[6];  // p, a, b, Gx, Gy, n: 2 B hex digits each
};

constexpr int kWideCurveCount = 6;
constexpr uint32_t kWideCofactor = 1;

static const WideCurveText kWideCurves[kWideCurveCount] = {
    {"secp384r1", 0, 48,
     {"fffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffeffffffff0000000000000000ffffffff",
      "fffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffeffffffff0000000000000000fffffffc",
      "b3312fa7e23ee7e4988e056be3f82d19181d9c6efe8141120314088f5013875ac656398d8a2ed19d2a85c8edd3ec2aef",
      "aa87ca22be8b05378eb1c71ef320ad746e1d3b628ba79b9859f741e082542a385502f25dbf55296c3a545e3872760ab7",
      "3617de4a96262c6f5d9e98bf9292dc29f8f41dbd289a147ce9da3113b5f0b8c00a60b1ce1d7e819d7a431d7c90ea0e5f",
      "ffffffffffffffffffffffffffffffffffffffffffffffffc7634d81f4372ddf581a0db248b0a77aecec196accc52973"}},
    {"brainpoolP384r1", 0, 48,
     {"8cb91e82a3386d280f5d6f7e50e641df152f7109ed5456b412b1da197fb71123acd3a729901d1a71874700133107ec53",
      "7bc382c63d8c150c3c72080ace05afa0c2bea28e4fb22787139165efba91f90f8aa5814a503ad4eb04a8c7dd22ce2826",
      "04a8c7dd22ce28268b39b55416f0447c2fb77de107dcd2a62e880ea53eeb62d57cb4390295dbc9943ab78696fa504c11",
      "1d1c64f068cf45ffa2a63a81b7c13f6b8847a3e77ef14fe3db7fcafe0cbd10e8e826e03436d646aaef87b2e247d4af1e",
      "8abe1d7520f9c2a45cb1eb8e95cfd55262b70b29feec5864e19c054ff99129280e4646217791811142820341263c5315",
      "8cb91e82a3386d280f5d6f7e50e641df152f7109ed5456b31f166e6cac0425a7cf3ab6af6b7fc3103b883202e9046565"}},
    {"brainpoolP512r1", 0, 64,
     {"aadd9db8dbe9c48b3fd4e6ae33c9fc07cb308db3b3c9d20ed6639cca703308717d4d9b009bc66842aecda12ae6a380e6"
      "2881ff2f2d82c68528aa6056583a48f3",
      "7830a3318b603b89e2327145ac234cc594cbdd8d3df91610a83441caea9863bc2ded5d5aa8253aa10a2ef1c98b9ac8b5"
      "7f1117a72bf2c7b9e7c1ac4d77fc94ca",
      "3df91610a83441caea9863bc2ded5d5aa8253aa10a2ef1c98b9ac8b57f1117a72bf2c7b9e7c1ac4d77fc94cadc083e67"
      "984050b75ebae5dd2809bd638016f723",
      "81aee4bdd82ed9645a21322e9c4c6a9385ed9f70b5d916c1b43b62eef4d0098eff3b1f78e2d0d48d50d1687b93b97d5f"
      "7c6d5047406a5e688b352209bcb9f822",
      "7dde385d566332ecc0eabfa9cf7822fdf209f70024a57b1aa000c55b881f8111b2dcde494a5f485e5bca4bd88a2763ae"
      "d1ca2b2fa8f0540678cd1e0f3ad80892",
      "aadd9db8dbe9c48b3fd4e6ae33c9fc07cb308db3b3c9d20ed6639cca70330870553e5c414ca92619418661197fac1047"
      "1db1d381085ddaddb58796829ca90069"}},
    {"id-tc26-gost-3410-12-512-paramSetA", 1, 64,
     {"ffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff"
      "fffffffffffffffffffffffffffffdc7",
      "ffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff"
      "fffffffffffffffffffffffffffffdc4",
      "e8c2505dedfc86ddc1bd0b2b6667f1da34b82574761cb0e879bd081cfd0b6265ee3cb090f30d27614cb4574010da90dd"
      "862ef9d4ebee4761503190785a71c760",
      "000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
      "00000000000000000000000000000003",
      "7503cfe87a836ae3a61b8816e25450e6ce5e1c93acf1abc1778064fdcbefa921df1626be4fd036e93d75e6a50e3a41e9"
      "8028fe5fc235f5b889a589cb5215f2a4",
      "ffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff27e69532f48d89116ff22b8d4e056060"
      "9b4b38abfad2b85dcacdb1411f10b275"}},
    {"id-tc26-gost-3410-12-512-paramSetB", 1, 64,
     {"800000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
      "0000000000000000000000000000006f",
      "800000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
      "0000000000000000000000000000006c",
      "687d1b459dc841457e3e06cf6f5e2517b97c7d614af138bcbf85dc806c4b289f3e965d2db1416d217f8b276fad1ab69c"
      "50f78bee1fa3106efb8ccbc7c5140116",
      "000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
      "00000000000000000000000000000002",
      "1a8f7eda389b094c2c071e3647a8940f3c123b697578c213be6dd9e6c8ec7335dcb228fd1edf4a39152cbcaaf8c03988"
      "28041055f94ceeec7e21340780fe41bd",
      "800000000000000000000000000000000000000000000000000000000000000149a1ec142565a545acfdb77bd9d40cfa"
      "8b996712101bea0ec6346c54374f25bd"}},
    {"id-tc26-gost-3410-2012-512-paramSetTest", 1, 64,
     {"4531acd1fe0023c7550d267b6b2fee80922b14b2ffb90f04d4eb7c09b5d2d15df1d852741af4704a0458047e80e4546d"
      "35b8336fac224dd81664bbf528be6373",
      "000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
      "00000000000000000000000000000007",
      "1cff0806a31116da29d8cfa54e57eb748bc5f377e49400fdd788b649eca1ac4361834013b2ad7322480a89ca58e0cf74"
      "bc9e540c2add6897fad0a3084f302adc",
      "24d19cc64572ee30f396bf6ebbfd7a6c5213b3b3d7057cc825f91093a68cd762fd60611262cd838dc6b60aa7eee804e2"
      "8bc849977fac33b4b530f1b120248a9a",
      "2bb312a43bd2ce6e0d020613c857acddcfbf061e91e5f2c3f32447c259f39b2c83ab156d77f1496bf7eb3351e1ee4e43"
      "dc1a18b91b24640b6dbb92cb1add371e",
      "4531acd1fe0023c7550d267b6b2fee80922b14b2ffb90f04d4eb7c09b5d2d15da82f2d7ecb1dbac719905c5eecc423f1"
      "d86e25edbe23c595d644aaf187e6e6df"}},
};

}  // namespace lcbec
