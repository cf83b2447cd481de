// gn_ref_check_main.cpp -- a host-only checker of the reference-order host algebra (gn_ref_host.h) with its own main: no HIP, no
// Python, built under AddressSanitizer + UBSan by `make gn_ref_check`.  Reads systems from a text file, one per line, every number as
// the hex word of its IEEE bit pattern, and prints the results the same way:
//   L6 <36 A> <6 b>   -> L6 <6 x>    refhost::ldlt_solve<double, 6>, row-major A, tmax = DBL_MAX
//   L3 <9 A> <3 b>    -> L3 <3 x>    refhost::ldlt_solve<float, 3>, tmax = FLT_MAX (32-bit words)
//   R  <3 w>          -> R  <9 R>    refhost::rodrigues
//   I  <16 m>         -> I  <16 o>   refhost::inv44
// tests/test_cpu_gn_ref_check.py compares the output with the oracle's statement of the same algebra bit for bit.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "gn_ref_host.h"

using namespace cf::refhost;

namespace {
template <class T, class U> bool read_words(char*& p, T* out, int n)
{
    for (int k = 0; k < n; k++) {
        char* end = nullptr;
        const unsigned long long v = strtoull(p, &end, 16);
        if (end == p) return false;
        const U u = (U)v;
        memcpy(&out[k], &u, sizeof(T));
        p = end;
    }
    return true;
}
template <class T, class U> void print_words(const char* tag, const T* v, int n)
{
    printf("%s", tag);
    for (int k = 0; k < n; k++) { U u; memcpy(&u, &v[k], sizeof(T)); printf(" %" PRIx64, (uint64_t)u); }
    printf("\n");
}
}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: gn_ref_check SYSTEMS.txt\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "gn_ref_check: cannot open %s\n", argv[1]); return 2; }
    std::vector<char> line(1 << 12);
    int n = 0;
    while (fgets(line.data(), (int)line.size(), f)) {
        char* p = line.data();
        char tag[4] = {0};
        int used = 0;
        if (sscanf(p, "%3s%n", tag, &used) != 1) continue;   // an empty line
        p += used;
        bool ok = false;
        if (!strcmp(tag, "L6")) {
            double A[36], b[6], x[6];
            ok = read_words<double, uint64_t>(p, A, 36) && read_words<double, uint64_t>(p, b, 6);
            if (ok) { ldlt_solve<double, 6>(A, b, x, DBL_MAX); print_words<double, uint64_t>("L6", x, 6); }
        } else if (!strcmp(tag, "L3")) {
            float A[9], b[3], x[3];
            ok = read_words<float, uint32_t>(p, A, 9) && read_words<float, uint32_t>(p, b, 3);
            if (ok) { ldlt_solve<float, 3>(A, b, x, FLT_MAX); print_words<float, uint32_t>("L3", x, 3); }
        } else if (!strcmp(tag, "R")) {
            double w[3], R[9];
            ok = read_words<double, uint64_t>(p, w, 3);
            if (ok) { rodrigues(w, R); print_words<double, uint64_t>("R", R, 9); }
        } else if (!strcmp(tag, "I")) {
            double m[16], o[16];
            ok = read_words<double, uint64_t>(p, m, 16);
            if (ok) { inv44(m, o); print_words<double, uint64_t>("I", o, 16); }
        }
        if (!ok) { fprintf(stderr, "gn_ref_check: line %d is malformed\n", n + 1); fclose(f); return 1; }
        n++;
    }
    fclose(f);
    fprintf(stderr, "gn_ref_check: %d systems\n", n);
    return 0;
}
