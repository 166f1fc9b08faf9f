// The files of the *_exact programs: a driver writes its case as little-endian 32-bit words to argv[1] and reads the words the
// program leaves in argv[2].  An I/O error ends the program with exit code 2, the code main gives a blob of the wrong size.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

// the whole file; *bytes is its size, the last word is zero-padded where that is no multiple of 4
static inline std::vector<uint32_t> read_words(const char* path, long* bytes = nullptr) {
    FILE* f = std::fopen(path, "rb");
    if (!f) std::exit(2);
    std::fseek(f, 0, SEEK_END);
    const long size = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<uint32_t> words((size_t)(size + 3) / 4);
    if (std::fread(words.data(), 1, (size_t)size, f) != (size_t)size) std::exit(2);
    std::fclose(f);
    if (bytes) *bytes = size;
    return words;
}

// words of either kind (uint32_t, float); `more` follows `words` in the file
template <class T, class U = uint32_t>
static inline void write_words(const char* path, const std::vector<T>& words, const std::vector<U>& more = {}) {
    static_assert(sizeof(T) == 4 && sizeof(U) == 4, "32-bit words");
    FILE* o = std::fopen(path, "wb");
    if (!o || std::fwrite(words.data(), 4, words.size(), o) != words.size() || std::fwrite(more.data(), 4, more.size(), o) != more.size() || std::fclose(o)) std::exit(2);
}
