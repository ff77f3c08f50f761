// stream_state_host.cpp — the host-only header liblcb_amd/csrc/stream_state.hpp
// as a stand-alone program (built with AddressSanitizer and UBSan by
// tests/test_stream_state_host.py; nothing is loaded into Python).
//
// stdin: records of (int32 set_alg, 344-byte lcb_hash_stream_state_t).  For
// each, one line: state_check's result and, when it is 0, the record after
// state_to_words -> words_to_state as hex (the context words sit in a heap
// block of exactly alg_words(alg) words, so a write past them is reported).
// Then one line "index" with index_check's results for a few lists.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../liblcb_amd/csrc/stream_state.hpp"

using namespace lcbstream;

int main() {
    static_assert(sizeof(lcb_hash_stream_state_t) == 344, "record size");
    for (;;) {
        int32_t alg;
        if (fread(&alg, 4, 1, stdin) != 1) break;
        lcb_hash_stream_state_t* r = (lcb_hash_stream_state_t*)malloc(sizeof(*r));
        if (fread(r, sizeof(*r), 1, stdin) != 1) return 2;
        const int rc = state_check(alg, *r);
        printf("%d", rc);
        if (rc == 0) {
            uint32_t* w = (uint32_t*)malloc(alg_words(alg) * 4);
            lcb_hash_stream_state_t* o = (lcb_hash_stream_state_t*)malloc(sizeof(*o));
            state_to_words(alg, *r, w);
            words_to_state(alg, w, *o);
            printf(" ");
            for (size_t i = 0; i < sizeof(*o); ++i) printf("%02x", ((const uint8_t*)o)[i]);
            free(o);
            free(w);
        }
        printf("\n");
        free(r);
    }
    std::vector<uint8_t> seen(5, 0);
    const uint32_t ok[] = {4, 0, 2}, past[] = {0, 5}, twice[] = {1, 3, 1}, rev[] = {4, 3, 2, 1, 0};
    printf("index %d %d %d %d %d %d", index_check(ok, 3, 5, seen.data()), index_check(past, 2, 5, seen.data()),
           index_check(twice, 3, 5, seen.data()), index_check(rev, 5, 5, seen.data()),
           index_check(nullptr, 5, 5, seen.data()), index_check(nullptr, 6, 5, seen.data()));
    for (uint8_t s : seen) printf(" %d", s);
    printf("\n");
    return 0;
}
