// Stencil kernel instances: the rank filters Median3/5, Erode3/5, Dilate3/5
// (k_rank, rank_kernels.h).
#include "rank_kernels.h"

namespace stripe {
namespace dev {

STRIPE_INSTANTIATE_LAUNCH_FILTER(Median3)
STRIPE_INSTANTIATE_LAUNCH_FILTER(Median5)
STRIPE_INSTANTIATE_LAUNCH_FILTER(Erode3)
STRIPE_INSTANTIATE_LAUNCH_FILTER(Erode5)
STRIPE_INSTANTIATE_LAUNCH_FILTER(Dilate3)
STRIPE_INSTANTIATE_LAUNCH_FILTER(Dilate5)

}  // namespace dev
}  // namespace stripe
