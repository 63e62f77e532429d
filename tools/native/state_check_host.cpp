// state_check_host.cpp - the rules of k_state_check (csrc/catan_state_check.h), the very lines the kernel compiles, built for the host:
//   g++ -std=c++17 -O1 -fsanitize=undefined,address -fno-sanitize-recover=all -I settlers_of_catan_rl_amd/csrc tools/native/state_check_host.cpp
//   state_check_host IN OUT      IN: int32 [m][736] blobs, OUT: uint64 [m] violation words
// Under the sanitizers a shift by an unchecked word, an index past an array or a signed overflow ends the run, which is how
// tests/test_state_check_host_cpu.py holds the kernel's source to "total on every input" without a GPU.
#include <stdint.h>
#include <stdio.h>
#include <vector>

#define DEVI inline
#define CATAN_TABLE static const
#define CATAN_FN static inline
#define CATAN_TOPOLOGY_CODE
#include "catan_topology.inc"
static inline int __popcll(unsigned long long x) { return __builtin_popcountll(x); }
static inline int __popc(unsigned x) { return __builtin_popcount(x); }
#define CATAN_STATE_CHECK_CODE
#include "catan_state_check.h"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    std::vector<int32_t> blob(catan::STATE_WORDS);
    std::vector<uint64_t> out;
    while (fread(blob.data(), sizeof(int32_t), blob.size(), in) == blob.size())
        out.push_back(catan::state_check_blob(catan::ScBlob{ blob.data(), 1, 0 }));
    fclose(in);
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    const bool ok = fwrite(out.data(), sizeof(uint64_t), out.size(), o) == out.size();
    return fclose(o) == 0 && ok ? 0 : 1;
}
