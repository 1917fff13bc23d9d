// tests/emul/order_io.h - the files the ordering / finishing unit harnesses (device_order.hip, wave_sort_form.cpp) exchange with
// their tests: a 32-bit count of sections, then per section a 64-bit byte count and the bytes (tests/order_cases.py writes and
// reads the same).  What a section holds is fixed by its position, case by case.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

struct Sections {
    std::vector<std::vector<uint8_t>> s;
    size_t next = 0;                                               // (reading: the section the next take() returns)
    template <class T> const T *take(size_t *count = nullptr)
    {
        if (next >= s.size()) { fprintf(stderr, "input: section %zu missing\n", next); exit(2); }
        const std::vector<uint8_t> &b = s[next++];
        if (b.size() % sizeof(T)) { fprintf(stderr, "input: section %zu is no array of %zu-byte elements\n", next - 1, sizeof(T)); exit(2); }
        if (count) *count = b.size() / sizeof(T);
        return (const T *)b.data();
    }
    template <class T> void put(const T *p, size_t count)
    {
        std::vector<uint8_t> b(count * sizeof(T));
        if (count) memcpy(b.data(), p, b.size());
        s.push_back(std::move(b));
    }
    template <class T> void put(const std::vector<T> &v) { put(v.data(), v.size()); }
};
inline Sections sections_read(const char *path)
{
    Sections S;
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    uint32_t ns = 0;
    if (fread(&ns, 4, 1, f) != 1) { fprintf(stderr, "%s: empty\n", path); exit(2); }
    for (uint32_t i = 0; i < ns; i++) {
        uint64_t nb = 0;
        if (fread(&nb, 8, 1, f) != 1) { fprintf(stderr, "%s: truncated\n", path); exit(2); }
        std::vector<uint8_t> b(nb);
        if (nb && fread(b.data(), 1, nb, f) != nb) { fprintf(stderr, "%s: truncated\n", path); exit(2); }
        S.s.push_back(std::move(b));
    }
    fclose(f);
    return S;
}
inline void sections_write(const char *path, const Sections &S)
{
    FILE *f = fopen(path, "wb");
    if (!f) { perror(path); exit(2); }
    const uint32_t ns = (uint32_t)S.s.size();
    fwrite(&ns, 4, 1, f);
    for (const std::vector<uint8_t> &b : S.s) { const uint64_t nb = b.size(); fwrite(&nb, 8, 1, f); if (nb) fwrite(b.data(), 1, nb, f); }
    if (fclose(f)) { perror(path); exit(2); }
}
