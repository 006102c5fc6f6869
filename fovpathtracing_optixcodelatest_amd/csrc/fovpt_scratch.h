// fovpt_scratch.h -- host only: the one owner of the device arrays a hierarchy build works in (bvh_build.hip).  Every array goes
// when the owner does and none sooner (hipFree waits for the device), except the one keep() takes out: the result.
#pragma once
#include <vector>

#include <hip/hip_runtime.h>

struct Scratch {
    std::vector<void*> held;
    Scratch() = default;
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() { for (void* p : held) if (p) (void)hipFree(p); }
    template <class T> hipError_t array(T** p, size_t count)
    {
        *p = nullptr;
        const hipError_t e = hipMalloc((void**)p, sizeof(T) * count);
        if (e == hipSuccess) held.push_back(*p);
        return e;
    }
    void keep(void* p) { for (void*& q : held) if (q == p) q = nullptr; }
};
