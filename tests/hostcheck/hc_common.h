// hc_common.h -- what the three host-check drivers share: the assertion that counts instead of aborting, key=value lookup in a describe line, "device" buffers.
#pragma once
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hc_stub.h"
#include "tsvpp.h"

namespace hc {

inline std::atomic<int> g_failed{ 0 };
inline std::atomic<long> g_checked{ 0 };

#define HC_CHECK(COND, ...)                                                          \
    do {                                                                             \
        hc::g_checked.fetch_add(1, std::memory_order_relaxed);                       \
        if (!(COND)) {                                                               \
            if (hc::g_failed.fetch_add(1) < 40) {                                    \
                std::fprintf(stderr, "%s:%d: FAILED %s: ", __FILE__, __LINE__, #COND); \
                std::fprintf(stderr, __VA_ARGS__);                                   \
                std::fputc('\n', stderr);                                            \
            }                                                                        \
        }                                                                            \
    } while (0)

// the value of `key` in a line of key=value pairs ("" if absent)
inline std::string value_of(const std::string &line, const char *key) {
    const std::string k = std::string(key) + "=";
    size_t at = 0;
    while ((at = line.find(k, at)) != std::string::npos) {
        if (at == 0 || line[at - 1] == ' ') {
            const size_t b = at + k.size(), e = line.find(' ', b);
            return line.substr(b, e == std::string::npos ? std::string::npos : e - b);
        }
        at += k.size();
    }
    return "";
}
inline long number_of(const std::string &line, const char *key) {
    const std::string v = value_of(line, key);
    return v.empty() ? -1 : std::atol(v.c_str());
}
// a describe line without the keys that depend on the request's size (tests/dispatch_grid.py: SIZE_KEYS)
inline std::string signature_of(const std::string &line) {
    std::string out;
    size_t b = 0;
    while (b < line.size()) {
        size_t e = line.find(' ', b);
        if (e == std::string::npos) e = line.size();
        const std::string item = line.substr(b, e - b);
        bool size_key = false;
        for (const char *k : { "src=", "dst=", "grid=", "tiles=", "frames=", "lds=" }) size_key = size_key || item.rfind(k, 0) == 0;
        if (!size_key) out += (out.empty() ? "" : " ") + item;
        b = e + 1;
    }
    return out;
}

// a "device" block of the stub's (256-byte aligned); the drivers free what they allocate: the stub's count of live blocks is part of the verdict
inline uint8_t *dev_alloc(size_t bytes) {
    void *p = nullptr;
    const hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
    if (e != hipSuccess || !p) {
        std::fprintf(stderr, "hostcheck: the stub refused a driver's own allocation of %zu bytes (%d)\n", bytes, (int)e);
        std::exit(3);
    }
    return (uint8_t *)p;
}

inline int current_device() {
    int d = -1;
    (void)hipGetDevice(&d);
    return d;
}

// a driver's exit status: 0 only without a failed assertion, a stub violation or anything the stub still holds
inline int verdict(const char *who) {
    const long bad = hc_stub_report(who);
    std::fprintf(stderr, "%s: %ld assertions, %d failed\n", who, g_checked.load(), g_failed.load());
    return (g_failed.load() || bad) ? 1 : 0;
}

} // namespace hc
