// conv_igemm.h's split-staged tiles in bf16x6: SplitTiles<2>
#include "conv_split_family.h"

namespace stemseg {

template int launch_split_family<2>(ConvKParams& p, const ConvKParams& d, const LaunchCtx& L, int tile_cfg, bool k3, bool k2);

}  // namespace stemseg
