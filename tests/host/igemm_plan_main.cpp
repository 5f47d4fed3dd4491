// edtr_amd/csrc/igemm_plan.h as a plain host program: no HIP header, no device, no library.  tests/test_igemm_plan_cpu.py compiles it
// under AddressSanitizer / UBSan and feeds it the generated cases.
//   stdin : one case per line, the bytes of an edtr_igemm_params as hex
//   stdout: "rc fast stagger debug_flags" per case, for the 256 CUs edtr_igemm_plan answers for
//   --time R: plan every case R times instead and print the nanoseconds per plan
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "igemm_plan.h"

static int nibble(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

int main(int argc, char** argv) {
    std::vector<edtr_igemm_params> cases;
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.size() != 2 * sizeof(edtr_igemm_params)) {
            fprintf(stderr, "case %zu: %zu hex digits, edtr_igemm_params has %zu bytes\n", cases.size(), line.size(), sizeof(edtr_igemm_params));
            return 2;
        }
        unsigned char raw[sizeof(edtr_igemm_params)];
        for (size_t i = 0; i < sizeof(raw); ++i) {
            const int hi = nibble(line[2 * i]), lo = nibble(line[2 * i + 1]);
            if (hi < 0 || lo < 0) return 2;
            raw[i] = (unsigned char)(hi * 16 + lo);
        }
        edtr_igemm_params p;
        memcpy(&p, raw, sizeof(p));
        cases.push_back(p);
    }
    if (argc == 3 && !strcmp(argv[1], "--time")) {
        const int rounds = atoi(argv[2]);
        long sum = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int r = 0; r < rounds; ++r)
            for (const edtr_igemm_params& p : cases) sum += igemm_plan::plan(&p, 256).rc;
        const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
        printf("%.2f ns per plan (%zu cases x %d, checksum %ld)\n", ns / ((double)rounds * cases.size()), cases.size(), rounds, sum);
        return 0;
    }
    for (const edtr_igemm_params& p : cases) {
        const igemm_plan::IgemmPlan pl = igemm_plan::plan(&p, 256);
        printf("%d %d %d %d\n", pl.rc, (int)pl.fast, pl.p.stagger, pl.p.debug_flags);
    }
    return 0;
}
