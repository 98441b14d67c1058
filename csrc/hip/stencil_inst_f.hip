// Stencil kernel instances: the bilateral filters Bilateral3/5
// (k_bilateral, bilateral_kernels.h).
#include "bilateral_kernels.h"

namespace stripe {
namespace dev {

STRIPE_INSTANTIATE_LAUNCH_FILTER(Bilateral3)
STRIPE_INSTANTIATE_LAUNCH_FILTER(Bilateral5)

}  // namespace dev
}  // namespace stripe
