// Device prefix scans with their temporary storage in a grow-only buffer: the size query,
// tmp.ensure, then the scan (the pattern of swps_sort.h's DevMem sorts).
#pragma once
#include <hipcub/hipcub.hpp>

#include "swps_internal.h"

namespace swps {

template <typename In, typename T>
int exclusive_scan(In in, T *out, uint64_t n, DevMem &tmp, hipStream_t s) {
  size_t b = 0;
  SWPS_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, b, in, out, (int)n, s));
  SWPS_TRY(tmp.ensure(b));
  b = tmp.bytes;
  SWPS_HIP(hipcub::DeviceScan::ExclusiveSum(tmp.p, b, in, out, (int)n, s));
  return SWPS_OK;
}
template <typename In, typename T> int inclusive_scan(In in, T *out, uint64_t n, DevMem &tmp, hipStream_t s) {
  size_t b = 0;
  SWPS_HIP(hipcub::DeviceScan::InclusiveSum(nullptr, b, in, out, (int)n, s));
  SWPS_TRY(tmp.ensure(b));
  b = tmp.bytes;
  SWPS_HIP(hipcub::DeviceScan::InclusiveSum(tmp.p, b, in, out, (int)n, s));
  return SWPS_OK;
}
// in place: io[i] = max(io[0..i])
template <typename T> int inclusive_max_scan(T *io, uint64_t n, DevMem &tmp, hipStream_t s) {
  size_t b = 0;
  SWPS_HIP(hipcub::DeviceScan::InclusiveScan(nullptr, b, io, io, hipcub::Max(), (int)n, s));
  SWPS_TRY(tmp.ensure(b));
  b = tmp.bytes;
  SWPS_HIP(hipcub::DeviceScan::InclusiveScan(tmp.p, b, io, io, hipcub::Max(), (int)n, s));
  return SWPS_OK;
}

}  // namespace swps
