// layer_refusals.cpp -- the host-side argument checks of the five `_layer` entry points (include/popcorn_hip.h), each refusal called once,
// as a stand-alone program for a sanitizer build of the HOST code (no GPU needed: every call returns PC_EINVAL before anything is enqueued):
//
//   cd popcorn_amd/csrc && hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -I../../include -Xarch_host -fsanitize=address,undefined \
//       train_ops.hip region.hip region_batch.hip region_crop.hip ../../tools/layer_refusals.cpp -o /tmp/layer_refusals && /tmp/layer_refusals
//
// Exit status 0 and "15 refusals, all PC_EINVAL" is the expected end; a sanitizer report ends the program with its own status.
#include <cstdint>
#include <cstdio>

#include "popcorn_hip.h"

int main() {
    // memory the checks may look at (they never dereference a device pointer): real host arrays, aligned for what they stand for
    alignas(16) static float f[64];
    alignas(16) static int32_t ib[64];
    static const int32_t band[6] = {0, 1, 2, 3, 0, 1};
    static const int32_t crop[5] = {1, 9, 2, 14, 0};
    static const float mean[6] = {0, 0, 0, 0, 0, 0}, stdv[6] = {1, 1, 1, 1, 1, 1};
    float* layer = f + 16;
    float* out = f + 32;
    float* odd = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(f + 48) + 1);      // & 3 != 0; never dereferenced
    int bad = 0, n = 0;
    auto expect = [&](const char* what, int code) {
        ++n;
        if (code != PC_EINVAL) { ++bad; std::printf("%s: returned %d, not PC_EINVAL\n", what, code); }
    };
    const float* ls[3] = {nullptr, layer, odd};
    float* os[3] = {out, nullptr, out};
    const char* why[3] = {"NULL layer with a layer output", "layer output without a layer", "misaligned layer"};
    for (int k = 0; k < 3; ++k) {
        char name[96];
        std::snprintf(name, sizeof name, "pc_augment_raw_layer (%s)", why[k]);
        expect(name, pc_augment_raw_layer(f, f, f, ls[k], f, f, os[k], 1, 8, 12, 0, 0, 0, 0, 1.f, 0, 1.f, nullptr));
        std::snprintf(name, sizeof name, "pc_region_gather_layer (%s)", why[k]);
        expect(name, pc_region_gather_layer(f, 0, f, nullptr, nullptr, ib, ls[k], 1, 4, 2, 16, 16, band, crop, 1, 8, 12, f, f, f, os[k], ib, nullptr));
        std::snprintf(name, sizeof name, "pc_region_batch_layer (%s)", why[k]);
        expect(name, pc_region_batch_layer(f, 0, f, nullptr, nullptr, ib, ls[k], 1, 4, 2, 16, 16, band, crop, 1, 8, 12, 0, 0, 0, 0, 1.f, 0, 1.f, f, f,
                                           os[k], 8, 12, nullptr, nullptr));
        std::snprintf(name, sizeof name, "pc_region_window_layer (%s)", why[k]);
        expect(name, pc_region_window_layer(f, 0, f, nullptr, 0, ls[k], 1, 4, 2, 16, 16, band, 2, 3, 0, 8, mean, stdv, nullptr, nullptr, 0, 0, 0, f,
                                            os[k], nullptr));
        std::snprintf(name, sizeof name, "pc_region_item_layer (%s)", why[k]);
        expect(name, pc_region_item_layer(f, 0, f, nullptr, 0, ib, ls[k], 1, 4, 2, 16, 16, band, 1, 9, 2, 14, 0, mean, stdv, nullptr, nullptr, 0, 0,
                                          0, f, f, os[k], nullptr));
    }
    std::printf("%d refusals, %s\n", n, bad ? "NOT all PC_EINVAL" : "all PC_EINVAL");
    return bad ? 1 : 0;
}
