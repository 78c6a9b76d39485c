// host_error.hpp -- the thread-local error message of libANN.so for host-only sources (no HIP headers), so they
// build and run stand-alone; the same declarations as tiler_common.hpp.
#pragma once

#include <string>

namespace tiler {
void set_error(const std::string &msg);
const char *last_error();
}  // namespace tiler
