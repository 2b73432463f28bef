// Host-visible launch interface of kernels_j2k_t1.hip: tier-1 of the JPEG 2000 decoder - the MQ arithmetic decoder and the
// three coding passes over every code block of a batch - to the integers of j2k::tier1 (host/j2k_decode.h), whose text it
// compiles.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../host/j2k_decode.h"  // t1::decode, the MQ decoder and its tables, stated once for host and device

namespace ocr {

constexpr int kJ2kT1Wave = 64;          // a code block belongs to one wavefront, and a workgroup is one wavefront
constexpr int kJ2kT1Samples = 4096;     // of a block at most (j2k::coded_fault)
constexpr int kJ2kT1FlagBytes = 6160;   // (w + 2) * (h + 2) <= 4096 + 2 * (1024 + 4) + 4 = 6156 for w * h <= 4096, w, h <= 1024
constexpr int kJ2kT1Window = 256;       // bytes of the segment staged in LDS at a time

struct J2kT1Block {  // a code block of the batch; every field checked on the host (j2k::coded_fault)
  uint32_t plane;     // where its top-left sample lies in plane a of the batch
  uint32_t stride;    // the tile-component's width
  uint32_t byte_off;  // into the batch's byte pool
  uint32_t byte_len;
  uint16_t w, h;
  uint8_t orient, numbps, passes, reserved;
};

// One workgroup a block, in the order of the list (the caller sorts it by passes * w * h, descending, so that the long
// blocks do not form the tail).  Writes w * h values of `plane` per block and nothing else.
void launch_j2k_t1(const J2kT1Block* blocks, uint32_t count, const uint8_t* pool, int32_t* plane, hipStream_t s);

}  // namespace ocr
