// The ABI tables (include/t3d.h: t3d_abi_entry, t3d_abi_struct): what every entry point takes and how every struct is laid
// out, made by the compiler from the header's own declarations.  Host code only -- no kernel, no HIP call, no allocation:
// every table below is a compile-time constant.
#include <cstddef>
#include <initializer_list>
#include <type_traits>

#include "../../include/t3d.h"
#include "abi_entries.h"

namespace {

// ---- entry points: one character per argument, from the declared function type ---------------------------------------
template <class T>
struct Unknown : std::false_type {};

template <class T>
constexpr char type_code() {
  using U = std::remove_cv_t<std::remove_pointer_t<T>>;
  if constexpr (std::is_pointer<T>::value) {
    // the structs a caller hands over as a struct of its own (ctypes refuses a Structure for a void* parameter)
    if constexpr (std::is_same<U, t3d_prologue>::value) return 'P';
    else if constexpr (std::is_same<U, t3d_bnbwd>::value) return 'B';
    else if constexpr (std::is_same<U, t3d_loss_cfg>::value) return 'L';
    else if constexpr (std::is_same<U, t3d_draw_style>::value) return 'S';
    else if constexpr (std::is_same<U, t3d_bn_fold>::value) return 'F';
    else {
      static_assert(!std::is_function<U>::value, "t3d.h: a function pointer is not a data pointer");
      return 'p';
    }
  } else if constexpr (std::is_same<T, int>::value) return 'i';
  else if constexpr (std::is_same<T, long long>::value) return 'l';
  else if constexpr (std::is_same<T, unsigned long long>::value) return 'u';
  else if constexpr (std::is_same<T, float>::value) return 'f';
  else if constexpr (std::is_same<T, double>::value) return 'd';
  else {
    static_assert(Unknown<T>::value, "t3d.h: an argument type the ABI table has no code for (see t3d_abi_entry)");
    return '?';
  }
}

template <class... A>
struct Types {
  static constexpr char str[sizeof...(A) + 1] = {type_code<A>()..., '\0'};
};
template <class... A>
constexpr const char* types_of(int (*)(A...)) { return Types<A...>::str; }

struct Entry { const char* name; const char* types; int in_step; };
#define T3D_S(fn) {#fn, types_of(&fn), 1},
#define T3D_Q(fn) {#fn, types_of(&fn), 0},
constexpr Entry kEntries[] = {T3D_ABI_ENTRIES(T3D_S, T3D_Q)};
#undef T3D_S
#undef T3D_Q
constexpr int kNumEntries = (int)(sizeof(kEntries) / sizeof(kEntries[0]));

// ---- structs: name, sizeof, and "field:offset:bytes,..." from offsetof / sizeof -----------------------------------------
struct Field { const char* name; size_t offset, bytes; };
struct Text { char s[640]; };

template <size_t N>
constexpr Text describe(const Field (&f)[N]) {
  Text t{};
  size_t n = 0;
  for (size_t i = 0; i < N; ++i) {
    if (i) t.s[n++] = ',';
    for (const char* c = f[i].name; *c; ++c) t.s[n++] = *c;
    for (size_t v : {f[i].offset, f[i].bytes}) {
      t.s[n++] = ':';
      size_t div = 1;
      while (v / div >= 10) div *= 10;
      for (; div; div /= 10) t.s[n++] = (char)('0' + v / div % 10);
    }
  }
  t.s[n] = '\0';          // (a description longer than Text does not compile: the index leaves the array)
  return t;
}

// T3D_STRUCT(t3d_x, F(a) F(b) ...): a misspelt or removed member is a compile error
#define F(m) {#m, offsetof(T3D_THIS, m), sizeof(T3D_THIS::m)},
#define T3D_STRUCT(type, members)                        \
  namespace layout_##type {                              \
  using T3D_THIS = type;                                 \
  constexpr Field fields[] = {members};                  \
  constexpr Text text = describe(fields);                \
  }
T3D_STRUCT(t3d_prologue, F(scale) F(shift) F(se) F(act) F(se_after_act))
T3D_STRUCT(t3d_bnbwd, F(alpha) F(beta) F(gamma) F(per_sample))
T3D_STRUCT(t3d_aug_sample, F(offset) F(h) F(w) F(flags) F(alpha) F(beta255) F(reserved) F(m))
T3D_STRUCT(t3d_aug_chain, F(n_ops) F(flags) F(kind) F(p) F(m2))
T3D_STRUCT(t3d_det_sample, F(offset) F(h) F(w) F(turns) F(left) F(top) F(cx0) F(cy0) F(cx1) F(cy1) F(flags) F(delta) F(alpha)
           F(sat) F(hue) F(perm) F(reserved))
T3D_STRUCT(t3d_jpeg_info, F(h) F(w) F(ncomp) F(sampling) F(mcus_x) F(mcus_y) F(seg_mcus) F(nseg) F(scan_offset) F(scan_bytes)
           F(reason) F(reserved) F(comp_dc) F(comp_ac) F(quant) F(dc_bits) F(dc_vals) F(ac_bits) F(ac_vals))
T3D_STRUCT(t3d_jpeg_seg, F(byte) F(pred) F(bit) F(reserved) F(mcu))
T3D_STRUCT(t3d_jpeg_item, F(file_offset) F(file_bytes) F(out_offset) F(block_offset) F(seg_offset) F(reserved))
T3D_STRUCT(t3d_loss_cfg, F(c_l1) F(c_mse) F(c_smoothl1) F(smoothl1_beta) F(c_add) F(c_diag) F(c_wing) F(wing_w) F(wing_eps)
           F(c_ce) F(lam_reg) F(lam_cls))
T3D_STRUCT(t3d_draw_style, F(rect_th) F(edge_th) F(kp_radius) F(font_scale) F(flags) F(colors))
T3D_STRUCT(t3d_bn_fold, F(kind) F(C) F(nrep) F(rstride) F(stats) F(count) F(gamma) F(beta) F(rm) F(rv) F(nbt) F(momentum)
           F(eps) F(o0) F(o1) F(o2) F(o3) F(o4) F(mean) F(invstd))
#undef T3D_STRUCT
#undef F

struct Struct { const char* name; int size; const char* fields; };
#define T3D_ROW(type) {#type, (int)sizeof(type), layout_##type::text.s},
constexpr Struct kStructs[] = {
    T3D_ROW(t3d_prologue) T3D_ROW(t3d_bnbwd) T3D_ROW(t3d_aug_sample) T3D_ROW(t3d_aug_chain) T3D_ROW(t3d_det_sample)
    T3D_ROW(t3d_jpeg_info) T3D_ROW(t3d_jpeg_seg) T3D_ROW(t3d_jpeg_item) T3D_ROW(t3d_loss_cfg) T3D_ROW(t3d_draw_style)
    T3D_ROW(t3d_bn_fold)};
#undef T3D_ROW
constexpr int kNumStructs = (int)(sizeof(kStructs) / sizeof(kStructs[0]));

}  // namespace

extern "C" int t3d_abi_entry(int index, const char** name, const char** types, int* in_step) {
  if (index < 0 || index >= kNumEntries) return T3D_ERR_ARG;
  if (name) *name = kEntries[index].name;
  if (types) *types = kEntries[index].types;
  if (in_step) *in_step = kEntries[index].in_step;
  return T3D_OK;
}

extern "C" int t3d_abi_struct(int index, const char** name, int* size, const char** fields) {
  if (index < 0 || index >= kNumStructs) return T3D_ERR_ARG;
  if (name) *name = kStructs[index].name;
  if (size) *size = kStructs[index].size;
  if (fields) *fields = kStructs[index].fields;
  return T3D_OK;
}
