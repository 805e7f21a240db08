/* <opencv2/imgproc/types_c.h> for tools/ref_tracking: the four conversion codes Tracking's Grab* members name. */
#ifndef JSORB_REF_TRACKING_OPENCV_TYPES_C_H
#define JSORB_REF_TRACKING_OPENCV_TYPES_C_H
enum { CV_BGR2GRAY = 6, CV_RGB2GRAY = 7, CV_BGRA2GRAY = 10, CV_RGBA2GRAY = 11 };
#endif
