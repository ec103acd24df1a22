// clip_lengths_selftest.cpp - the length checks of the per-clip BiCodec calls (csrc/clip_lengths.h) as a stand-alone
// host program for the host sanitizers.  The length vectors live in exact-size heap blocks, so a read past either end is a report.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
//       -I include -I unified_audio_amd/csrc tools/clip_lengths_selftest.cpp -o /tmp/clip_lengths_selftest && /tmp/clip_lengths_selftest
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "clip_lengths.h"

static char g_error[512];
namespace qa {
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}
}  // namespace qa

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "%s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, g_error); \
            return 1;                                                            \
        }                                                                        \
    } while (0)

static int run(int64_t B, const int64_t* values, int64_t lo, int64_t hi, std::vector<int>* out, bool* full) {
    std::unique_ptr<int64_t[]> v(new int64_t[(size_t)(B > 0 ? B : 1)]);  // exact size: B entries and not one more
    if (B > 0) std::memcpy(v.get(), values, sizeof(int64_t) * (size_t)B);
    g_error[0] = 0;
    return qa::check_clip_lengths("selftest", B, v.get(), lo, hi, "tokens", "T", out, full);
}

int main() {
    std::vector<int> out;
    bool full = false;
    {
        const int64_t v[] = {37, 20, 7, 1};
        CHECK(run(4, v, 1, 37, &out, &full) == QA_OK && !full && out.size() == 4 && out[0] == 37 && out[3] == 1);
    }
    {
        const int64_t v[] = {37, 37, 37};
        CHECK(run(3, v, 1, 37, &out, &full) == QA_OK && full && out.size() == 3);
    }
    {
        const int64_t v[] = {1};
        CHECK(run(1, v, 1, 1, &out, &full) == QA_OK && full);
    }
    const struct {
        int64_t v[3];
        int row;
    } bad[] = {{{37, 0, 5}, 1}, {{38, 1, 1}, 0}, {{5, 5, -3}, 2}, {{INT64_MAX, 1, 1}, 0}, {{1, INT64_MIN, 1}, 1}};
    for (const auto& c : bad) {
        CHECK(run(3, c.v, 1, 37, &out, &full) == QA_ERR_INVALID);
        const std::string want = "selftest: lengths[" + std::to_string(c.row) + "] = " + std::to_string((long long)c.v[c.row]) + " is outside 1 .. T = 37";
        CHECK(std::strstr(g_error, want.c_str()) != nullptr);
    }
    {
        const int64_t v[] = {399, 400};
        CHECK(run(2, v, 400, 11577, &out, &full) == QA_ERR_INVALID && std::strstr(g_error, "lengths[0] = 399 is outside 400 .. T = 11577"));
    }
    {  // a batch size or an extent that cannot be a launch: refused before the vector is read
        const int64_t v[] = {1};
        CHECK(run(0, v, 1, 37, &out, &full) == QA_ERR_INVALID);
        CHECK(run(-4, v, 1, 37, &out, &full) == QA_ERR_INVALID);
        CHECK(run(1, v, 1, (int64_t)INT32_MAX + 1, &out, &full) == QA_ERR_INVALID);
        CHECK(run(1, v, 2, 1, &out, &full) == QA_ERR_INVALID);
        CHECK(qa::check_clip_lengths("selftest", 1, nullptr, 1, 37, "tokens", "T", &out, &full) == QA_ERR_INVALID);
        CHECK(qa::check_clip_lengths("selftest", 1, v, 1, 37, "tokens", "T", nullptr, &full) == QA_ERR_INVALID);
    }
    {  // the largest batch the check admits, every entry read exactly once
        const int64_t B = (1 << 20) - 1;
        std::vector<int64_t> v((size_t)B, 9);
        v.shrink_to_fit();
        v[(size_t)B - 1] = 10;
        g_error[0] = 0;
        CHECK(qa::check_clip_lengths("selftest", B, v.data(), 1, 9, "tokens", "T", &out, &full) == QA_ERR_INVALID);
        CHECK(std::strstr(g_error, "lengths[1048574] = 10"));
        v[(size_t)B - 1] = 9;
        CHECK(qa::check_clip_lengths("selftest", B, v.data(), 1, 9, "tokens", "T", &out, &full) == QA_OK && full && (int64_t)out.size() == B);
    }
    std::puts("clip_lengths_selftest ok");
    return 0;
}
