// radius_parse_host.cpp — the packet walk of the batched RADIUS sign/verify
// (liblcb_amd/csrc/radius_parse.hpp, the text the parse kernel compiles) as a
// host program, for a sanitizer build: tests/test_radius_parse_host.py builds
// it with -fsanitize=address,undefined and feeds it packets on stdin.
//
// Input: records of  u32 buf_size | u32 key_index | u32 nkeys | u32 req_code |
// buf_size bytes  (little-endian).  Every packet is copied into a heap block of
// exactly buf_size bytes, so a read past the buffer is an ASan report.
// Output: one line per record,
//   err len ma_off ma_len pw_off pw_len kidx sign_static e1 e2 e3 ma pass au pass pw pass ma_auth au_auth
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../liblcb_amd/csrc/radius_parse.hpp"

int main() {
    uint32_t hdr[4];
    while (fread(hdr, sizeof(hdr), 1, stdin) == 1) {
        const uint32_t n = hdr[0];
        uint8_t* p = static_cast<uint8_t*>(malloc(n));
        if (n && (!p || fread(p, 1, n, stdin) != n)) return 2;
        lcbrad::RadRec r;
        lcbrad::rad_parse(p, n, hdr[1], hdr[2], &r);
        int sign_static = 0;
        uint32_t aux = 0;
        if (!r.err) {
            sign_static = lcbrad::rad_sign_static(r);
            aux = lcbrad::rad_verify_plan(r, p[0], hdr[3]);
        }
        printf("%d %u %u %u %u %u %u %d %u %u %u %u %u %u %u %u\n", r.err, r.len, r.ma_off, r.ma_len, r.pw_off,
               r.pw_len, r.kidx, sign_static, lcbrad::plan_e1(aux), lcbrad::plan_e2(aux), lcbrad::plan_e3(aux),
               (aux & lcbrad::kPlanMa) ? 1u : 0u, (aux & lcbrad::kPlanAu) ? 1u : 0u, (aux & lcbrad::kPlanPw) ? 1u : 0u,
               lcbrad::plan_ma_auth(aux), lcbrad::plan_au_auth(aux));
        free(p);
    }
    return 0;
}
