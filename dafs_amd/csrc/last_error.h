// dafs_amd/csrc/last_error.h -- the setter of the thread's dafs_hip_last_error() text.  capi.cpp owns the string; host-only
// translation units (host_text.cpp) include this and nothing from HIP.
#pragma once

namespace dafs {
void set_last_error(const char* msg);
}
