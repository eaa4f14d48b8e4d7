// qhuff_names.h -- name lengths of the QPACK static table (RFC 9204
// Appendix A; the reference's static_table[], lsqpack.c:104-209 -- the list
// in tests/golden/qpack_static_table.json, which test_frames.py checks this
// against through qhuff_decode_literals_ex).  Plain C++: read by the host
// framing (qhuff_frames.cpp field_ref_name_len) and by the in-place literal
// decode's kernel, whose code object holds a copy (qhuff_wire_impl.h
// kWireNames, wire_ref_name_len).
#pragma once

#include <stdint.h>

namespace qhuff {

constexpr uint32_t kStaticNames = 99;
constexpr uint32_t kStaticNameMax = 32;      // the longest of them
constexpr uint8_t kStaticNameLen[kStaticNames] = {
    10, 5, 3, 19, 14, 6, 4, 4, 17, 13, 13, 4, 8, 7, 10, 7, 7, 7, 7, 7, 7, 7,
    7, 7, 7, 7, 7, 7, 7, 6, 6, 15, 13, 28, 28, 27, 13, 13, 13, 13, 13, 13,
    16, 16, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 5, 25, 25, 25, 4, 4,
    22, 16, 7, 7, 7, 7, 7, 7, 7, 7, 7, 15, 32, 32, 28, 28, 28, 28, 29, 30,
    29, 29, 7, 13, 23, 10, 9, 9, 8, 6, 7, 6, 19, 25, 10, 15, 15, 15};

constexpr bool
static_names_within(uint32_t i = 0)
{
    return i == kStaticNames
        || (kStaticNameLen[i] <= kStaticNameMax && static_names_within(i + 1));
}
static_assert(static_names_within(), "kStaticNameMax bounds every name");

}  // namespace qhuff
