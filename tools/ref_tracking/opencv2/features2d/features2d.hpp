/* <opencv2/features2d/features2d.hpp> for tools/ref_tracking: nothing of it is used. */
