// row_kind.h -- the storage kind of a handle's original-space rows, stated once.  Host and device code (no HIP header needed).
//   F32  gbnns_index_create            float32 rows
//   U8   gbnns_index_create_bytes      uint8 rows    ("byte handle")
//   F16  gbnns_index_create_half_base  binary16 rows ("half-base handle")
// Every row is padded with zeros to a multiple of 16 bytes; a handle's d_pad counts ELEMENTS of its kind (= the floats of a staged query).
#pragma once

#include <cstdint>

namespace gbnns {

enum class RowKind : uint8_t { F32, U8, F16 };

constexpr uint32_t row_elem_bytes(RowKind k) { return k == RowKind::U8 ? 1u : (k == RowKind::F16 ? 2u : 4u); }
constexpr uint32_t row_pad_elems(RowKind k) { return 16u / row_elem_bytes(k); }  // 4 / 16 / 8
constexpr uint32_t row_pad(uint32_t d, RowKind k) { return (d + row_pad_elems(k) - 1u) / row_pad_elems(k) * row_pad_elems(k); }
// for messages: "byte handle" / "half-base handle", and the function that creates one
constexpr const char* row_handle_noun(RowKind k) { return k == RowKind::U8 ? "byte handle" : (k == RowKind::F16 ? "half-base handle" : "float handle"); }
constexpr const char* row_create_fn(RowKind k) {
    return k == RowKind::U8 ? "gbnns_index_create_bytes" : (k == RowKind::F16 ? "gbnns_index_create_half_base" : "gbnns_index_create");
}
// ... and the name of that function's table argument
constexpr const char* row_table_arg(RowKind k) { return k == RowKind::U8 ? "db_bytes" : (k == RowKind::F16 ? "db_half" : "db"); }

}  // namespace gbnns
