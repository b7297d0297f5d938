// launch_check.h — the one post-launch error check shared by every .hip file.
#pragma once

#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

namespace auron {

// raise launch-configuration errors loudly (hipLaunchKernelGGL itself
// reports nothing)
inline void check_launch(const char* name) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    throw std::runtime_error(std::string("kernel launch failed: ") + name +
                             ": " + hipGetErrorString(e));
}

}  // namespace auron
