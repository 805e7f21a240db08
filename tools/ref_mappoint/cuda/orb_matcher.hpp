/* "cuda/orb_matcher.hpp" for tools/ref_mappoint: the project's stand-in, as it is (found here before the reference's CUDA header) */
#include "../../../oracle/ref_matcher/cuda/orb_matcher.hpp"
