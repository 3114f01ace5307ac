// Geometry of one stride-2 convolution layer of the frame video encoder's backbone, from the rules of include/mmdeer_frames.h;
// shared by the forward (conv2d.hip) and the backward (conv2d_bwd.hip).
#pragma once

namespace mmdeer {
namespace {

struct ConvGeom {
  int Hp, Wp, Cp, OH, OW, k;
};

// geometry of one layer, from the header's rules; false: unsupported (k, Cin)
inline bool conv_geom(int H, int W, int Cin, int k, int act_f32, ConvGeom& g, int& KWe) {
  const int epc = act_f32 ? 4 : 8;
  if (k == 7 && Cin == 3) { g.Cp = epc; KWe = 8; }
  else if (k == 3 && Cin > 0 && Cin % epc == 0) { g.Cp = Cin; KWe = 3; }
  else return false;
  const int p = k / 2;
  g.k = k; g.Hp = H + 2 * p; g.Wp = W + 2 * p;
  g.OH = (H + 2 * p - k) / 2 + 1; g.OW = (W + 2 * p - k) / 2 + 1;
  return true;
}

}  // namespace
}  // namespace mmdeer
