/* FNV-1a-64 over a byte range, continuing from h: what tests/host_san/driver.cpp computes per call line, for
 * tests/host_san_cases.py (a byte loop in Python would take minutes over the catalogue's plans). */
#include <stddef.h>
#include <stdint.h>

uint64_t fnv1a64(uint64_t h, const void* p, size_t n) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}
