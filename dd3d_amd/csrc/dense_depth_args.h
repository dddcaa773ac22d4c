// The conditions on dd3d_dense_depth_loss_args that the loss (dense_depth_loss.hip) and its gradient (dense_depth_loss_grads.hip) share.
#pragma once
#include "common.h"

namespace dd3d {

// `who`: the entry point's name, for the message.
inline int check_dense_depth_args(const dd3d_dense_depth_loss_args* a, const char* who) {
  DD3D_REQUIRE(a != nullptr, "%s: null args", who);
  DD3D_REQUIRE(a->num_levels >= 1 && a->num_levels <= DD3D_MAX_LEVELS, "%s: num_levels = %d outside [1, %d]", who, a->num_levels, DD3D_MAX_LEVELS);
  DD3D_REQUIRE(a->gt && a->partials && a->out && a->count, "%s: null buffer", who);
  DD3D_REQUIRE(a->B >= 1 && a->Hp >= 1 && a->Wp >= 4 && (a->Wp % 4) == 0 && a->pitch >= 1, "%s: B = %d, Hp = %d, Wp = %d (a multiple of 4), pitch = %d", who,
               a->B, a->Hp, a->Wp, a->pitch);
  DD3D_REQUIRE(a->Hp < (1 << 23) && a->Wp < (1 << 23), "%s: canvas %d x %d: a side must stay below 2^23 (f32 source coordinates)", who, a->Hp, a->Wp);
  DD3D_REQUIRE((reinterpret_cast<uintptr_t>(a->gt) & 15) == 0, "%s: the ground-truth canvas must be 16-byte aligned", who);
  DD3D_REQUIRE(a->focal_factor <= 0.f || a->inv_K, "%s: focal scaling needs inv_K", who);
  for (int l = 0; l < a->num_levels; ++l) {
    DD3D_REQUIRE(a->raw[l] != nullptr, "%s: level %d has no map", who, l);
    DD3D_REQUIRE(a->h[l] >= 1 && a->w[l] >= 1 && a->stride[l] >= 1 && (long)a->h[l] * a->stride[l] == a->Hp && (long)a->w[l] * a->stride[l] == a->Wp,
                 "%s: level %d (%d x %d, stride %d) does not tile the %d x %d canvas", who, l, a->h[l], a->w[l], a->stride[l], a->Hp, a->Wp);
  }
  return DD3D_OK;
}

}  // namespace dd3d
