/* <opencv2/features2d/features2d.hpp> for tools/ref_covis: cv::KeyPoint is in the core double */
#include <opencv2/core/core.hpp>
