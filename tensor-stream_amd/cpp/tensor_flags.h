// tensor_flags.h -- the optional tensor arguments of the check programs vpp_rois and vpp_letterbox, parsed in one place.
#pragma once
#include <cstdio>
#include <cstring>

#include "tsvpp.h"

#define TENSOR_FLAGS_USAGE "[--dtype f16|bf16|f32] [--mean a,b,c] [--scale a,b,c]"

// [--dtype f16|bf16|f32] [--mean a,b,c] [--scale a,b,c] in front of the positional arguments: fills `spec` (defaults: f32, mean 0, scale 1) and returns
// true when any was given; the arguments are shifted past the flags.
static inline bool tensor_flags(int &argc, char **&argv, tsvpp_tensor_spec &spec) {
    spec = tsvpp_tensor_spec{ TSVPP_F32, { 0.f, 0.f, 0.f }, { 1.f, 1.f, 1.f } };
    bool any = false;
    while (argc > 2 && (strcmp(argv[1], "--dtype") == 0 || strcmp(argv[1], "--mean") == 0 || strcmp(argv[1], "--scale") == 0)) {
        const char *v = argv[2];
        if (strcmp(argv[1], "--dtype") == 0) spec.dtype = strcmp(v, "f16") == 0 ? TSVPP_F16 : (strcmp(v, "bf16") == 0 ? TSVPP_BF16 : (strcmp(v, "f32") == 0 ? TSVPP_F32 : -1));
        else {
            float *dst = strcmp(argv[1], "--mean") == 0 ? spec.mean : spec.scale;
            if (sscanf(v, "%f,%f,%f", dst, dst + 1, dst + 2) != 3) dst[0] = dst[1] = dst[2] = __builtin_nanf(""); // (refused by the library: TSVPP_ERROR)
        }
        any = true;
        argv += 2;
        argc -= 2;
    }
    return any;
}
