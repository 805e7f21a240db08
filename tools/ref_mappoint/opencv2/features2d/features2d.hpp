/* <opencv2/features2d/features2d.hpp> for tools/ref_mappoint: the project's stand-in, as it is */
#include "../../../../oracle/ref_matcher/opencv2/features2d/features2d.hpp"
