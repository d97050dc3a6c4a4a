// common prologue of every kernel translation unit
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "cone_engine.h"
#include "ce_types.h"

// raise the dynamic-LDS limit of one kernel
template <class K>
inline hipError_t ce_set_max_lds(K *kernel, int bytes) { return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes); }
