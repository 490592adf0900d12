// conv_igemm.h's split-staged tiles in f16x3: SplitTiles<3> and the stem's 4x4 tile
#include "conv_split_family.h"

namespace stemseg {

template int launch_split_family<3>(ConvKParams& p, const ConvKParams& d, const LaunchCtx& L, int tile_cfg, bool k3, bool k2);

int launch_stem_f16x3(const ConvKParams& p, const LaunchCtx& L) { return launch_cfg<SplitTiles<3>::Y4Stem>(p, L.without_scratch()); }

}  // namespace stemseg
