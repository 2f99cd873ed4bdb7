// Sensor noise on 8-bit RGB images (`train --aug_noise / --aug_noise_shot`; not in the reference): read noise, constant over the tonal
// range, plus shot noise whose variance grows with the signal -- the heteroscedastic-Gaussian (Poisson-Gaussian) sensor model, per channel
// and pixel, independent, in the 8-bit domain of the network input.  No gamma is modelled: the variance is linear in the ENCODED level, not
// in the scene's light; that is the model's limit.  All integer, restated byte for byte by tests/noise_ref.py:
//     o       = (y W + x) 3 + c, the byte's offset from the first byte of ITS image;
//     word(o) = Philox4x32-10(counter = (o >> 2, 0, 0, 0), key = (k0, k1))[o & 3]   (Salmon et al., Random123: multipliers 0xD2511F53 on
//               counter word 0 and 0xCD9E8D57 on word 2, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds) -- one call serves four
//               successive bytes; H W < 2^31 keeps o >> 2 inside counter word 0;
//     z       = the unit normal in Q10 from the word's TOP 12 bits i = word >> 20 (the other 20 bits are not used):
//               z = H[i - 2048] if i >= 2048 else -H[2047 - i], H[j] = round(1024 Phi^-1((2048 + j + 0.5) / 4096)), the half table below
//               (tools/noise_table.py writes it; H[0] = 0, H[2047] = 3756);
//     sigma(v) = isqrt(a' + b' v) in Q8 for the grey level v, a' = min(a, 2^26), b' = min(b, 2^17): a = the read-noise variance in Q16
//               levels^2 (sigma_read <= 32 levels), b = the shot gain in Q16 levels^2 per level (gain <= 2), both read as uint32;
//     out     = clamp(v + ((z sigma(v) + 2^17) >> 18), 0, 255), an arithmetic shift; |z sigma| <= 3756 * 10026 < 2^31.
// table (B, 4) int32 on the device: [k0, k1, a, b].  The table cannot be checked without a sync: the clamps are part of the definition, every
// table index is a byte or a 12-bit field and nothing in a row decides an address, so any table is safe.  A row with a' = b' = 0 is the
// identity.  The bytes are a function of (image content, row) alone: not of the launch shape, the batch position or the base address.
//
// One launch, no workspace.  k_noise_u8: block (x, b) owns the NOISE_STRIP_BYTES bytes of image b from x NOISE_STRIP_BYTES on, cut into
// image-relative 16-byte chunks, i.e. four Philox calls each.  The prologue reads the row -- an identity row in place leaves at once --,
// builds the 256 sigmas (a float square root corrected by +-1 in integers) and stages H, 4.5 KB of LDS together.  A thread then takes a
// chunk a step: one 16-byte load where the image's first byte lies on a 16-byte boundary in `in` and in `out` (else 16 byte loads), four
// calls, 2 x 16 LDS gathers, one 16-byte store (else 16 byte stores).  The last block of an image maps the < 16 bytes behind the last whole
// chunk, a byte a thread.  Every byte is read and written by the same thread, so out may be in.
#include "sd_common.h"

// clang-format off
// ---- begin generated: tools/noise_table.py ----
#define SD_NOISE_HALF_TABLE \
       0,    1,    2,    2,    3,    3,    4,    5,    5,    6,    7,    7,    8,    8,    9,   10, \
      10,   11,   12,   12,   13,   13,   14,   15,   15,   16,   17,   17,   18,   18,   19,   20, \
      20,   21,   22,   22,   23,   24,   24,   25,   25,   26,   27,   27,   28,   29,   29,   30, \
      30,   31,   32,   32,   33,   34,   34,   35,   35,   36,   37,   37,   38,   39,   39,   40, \
      40,   41,   42,   42,   43,   44,   44,   45,   45,   46,   47,   47,   48,   49,   49,   50, \
      50,   51,   52,   52,   53,   54,   54,   55,   55,   56,   57,   57,   58,   59,   59,   60, \
      61,   61,   62,   62,   63,   64,   64,   65,   66,   66,   67,   67,   68,   69,   69,   70, \
      71,   71,   72,   72,   73,   74,   74,   75,   76,   76,   77,   77,   78,   79,   79,   80, \
      81,   81,   82,   82,   83,   84,   84,   85,   86,   86,   87,   88,   88,   89,   89,   90, \
      91,   91,   92,   93,   93,   94,   94,   95,   96,   96,   97,   98,   98,   99,   99,  100, \
     101,  101,  102,  103,  103,  104,  105,  105,  106,  106,  107,  108,  108,  109,  110,  110, \
     111,  111,  112,  113,  113,  114,  115,  115,  116,  116,  117,  118,  118,  119,  120,  120, \
     121,  122,  122,  123,  123,  124,  125,  125,  126,  127,  127,  128,  128,  129,  130,  130, \
     131,  132,  132,  133,  134,  134,  135,  135,  136,  137,  137,  138,  139,  139,  140,  140, \
     141,  142,  142,  143,  144,  144,  145,  146,  146,  147,  147,  148,  149,  149,  150,  151, \
     151,  152,  153,  153,  154,  154,  155,  156,  156,  157,  158,  158,  159,  160,  160,  161, \
     161,  162,  163,  163,  164,  165,  165,  166,  166,  167,  168,  168,  169,  170,  170,  171, \
     172,  172,  173,  173,  174,  175,  175,  176,  177,  177,  178,  179,  179,  180,  180,  181, \
     182,  182,  183,  184,  184,  185,  186,  186,  187,  187,  188,  189,  189,  190,  191,  191, \
     192,  193,  193,  194,  194,  195,  196,  196,  197,  198,  198,  199,  200,  200,  201,  202, \
     202,  203,  203,  204,  205,  205,  206,  207,  207,  208,  209,  209,  210,  210,  211,  212, \
     212,  213,  214,  214,  215,  216,  216,  217,  218,  218,  219,  219,  220,  221,  221,  222, \
     223,  223,  224,  225,  225,  226,  226,  227,  228,  228,  229,  230,  230,  231,  232,  232, \
     233,  234,  234,  235,  235,  236,  237,  237,  238,  239,  239,  240,  241,  241,  242,  243, \
     243,  244,  245,  245,  246,  246,  247,  248,  248,  249,  250,  250,  251,  252,  252,  253, \
     254,  254,  255,  255,  256,  257,  257,  258,  259,  259,  260,  261,  261,  262,  263,  263, \
     264,  265,  265,  266,  266,  267,  268,  268,  269,  270,  270,  271,  272,  272,  273,  274, \
     274,  275,  276,  276,  277,  278,  278,  279,  279,  280,  281,  281,  282,  283,  283,  284, \
     285,  285,  286,  287,  287,  288,  289,  289,  290,  291,  291,  292,  293,  293,  294,  294, \
     295,  296,  296,  297,  298,  298,  299,  300,  300,  301,  302,  302,  303,  304,  304,  305, \
     306,  306,  307,  308,  308,  309,  310,  310,  311,  311,  312,  313,  313,  314,  315,  315, \
     316,  317,  317,  318,  319,  319,  320,  321,  321,  322,  323,  323,  324,  325,  325,  326, \
     327,  327,  328,  329,  329,  330,  331,  331,  332,  333,  333,  334,  335,  335,  336,  337, \
     337,  338,  339,  339,  340,  340,  341,  342,  342,  343,  344,  344,  345,  346,  346,  347, \
     348,  348,  349,  350,  350,  351,  352,  352,  353,  354,  354,  355,  356,  356,  357,  358, \
     358,  359,  360,  360,  361,  362,  362,  363,  364,  364,  365,  366,  366,  367,  368,  368, \
     369,  370,  370,  371,  372,  372,  373,  374,  374,  375,  376,  376,  377,  378,  378,  379, \
     380,  380,  381,  382,  383,  383,  384,  385,  385,  386,  387,  387,  388,  389,  389,  390, \
     391,  391,  392,  393,  393,  394,  395,  395,  396,  397,  397,  398,  399,  399,  400,  401, \
     401,  402,  403,  403,  404,  405,  405,  406,  407,  407,  408,  409,  410,  410,  411,  412, \
     412,  413,  414,  414,  415,  416,  416,  417,  418,  418,  419,  420,  420,  421,  422,  422, \
     423,  424,  425,  425,  426,  427,  427,  428,  429,  429,  430,  431,  431,  432,  433,  433, \
     434,  435,  435,  436,  437,  438,  438,  439,  440,  440,  441,  442,  442,  443,  444,  444, \
     445,  446,  446,  447,  448,  449,  449,  450,  451,  451,  452,  453,  453,  454,  455,  455, \
     456,  457,  458,  458,  459,  460,  460,  461,  462,  462,  463,  464,  464,  465,  466,  467, \
     467,  468,  469,  469,  470,  471,  471,  472,  473,  473,  474,  475,  476,  476,  477,  478, \
     478,  479,  480,  480,  481,  482,  483,  483,  484,  485,  485,  486,  487,  487,  488,  489, \
     490,  490,  491,  492,  492,  493,  494,  495,  495,  496,  497,  497,  498,  499,  499,  500, \
     501,  502,  502,  503,  504,  504,  505,  506,  507,  507,  508,  509,  509,  510,  511,  511, \
     512,  513,  514,  514,  515,  516,  516,  517,  518,  519,  519,  520,  521,  521,  522,  523, \
     524,  524,  525,  526,  526,  527,  528,  529,  529,  530,  531,  531,  532,  533,  534,  534, \
     535,  536,  536,  537,  538,  539,  539,  540,  541,  542,  542,  543,  544,  544,  545,  546, \
     547,  547,  548,  549,  549,  550,  551,  552,  552,  553,  554,  555,  555,  556,  557,  557, \
     558,  559,  560,  560,  561,  562,  563,  563,  564,  565,  565,  566,  567,  568,  568,  569, \
     570,  571,  571,  572,  573,  574,  574,  575,  576,  576,  577,  578,  579,  579,  580,  581, \
     582,  582,  583,  584,  585,  585,  586,  587,  587,  588,  589,  590,  590,  591,  592,  593, \
     593,  594,  595,  596,  596,  597,  598,  599,  599,  600,  601,  602,  602,  603,  604,  605, \
     605,  606,  607,  608,  608,  609,  610,  611,  611,  612,  613,  614,  614,  615,  616,  617, \
     617,  618,  619,  620,  620,  621,  622,  623,  623,  624,  625,  626,  626,  627,  628,  629, \
     629,  630,  631,  632,  632,  633,  634,  635,  635,  636,  637,  638,  638,  639,  640,  641, \
     642,  642,  643,  644,  645,  645,  646,  647,  648,  648,  649,  650,  651,  651,  652,  653, \
     654,  655,  655,  656,  657,  658,  658,  659,  660,  661,  661,  662,  663,  664,  665,  665, \
     666,  667,  668,  668,  669,  670,  671,  672,  672,  673,  674,  675,  675,  676,  677,  678, \
     679,  679,  680,  681,  682,  682,  683,  684,  685,  686,  686,  687,  688,  689,  689,  690, \
     691,  692,  693,  693,  694,  695,  696,  697,  697,  698,  699,  700,  701,  701,  702,  703, \
     704,  705,  705,  706,  707,  708,  708,  709,  710,  711,  712,  712,  713,  714,  715,  716, \
     716,  717,  718,  719,  720,  720,  721,  722,  723,  724,  724,  725,  726,  727,  728,  729, \
     729,  730,  731,  732,  733,  733,  734,  735,  736,  737,  737,  738,  739,  740,  741,  741, \
     742,  743,  744,  745,  746,  746,  747,  748,  749,  750,  750,  751,  752,  753,  754,  755, \
     755,  756,  757,  758,  759,  760,  760,  761,  762,  763,  764,  764,  765,  766,  767,  768, \
     769,  769,  770,  771,  772,  773,  774,  774,  775,  776,  777,  778,  779,  779,  780,  781, \
     782,  783,  784,  785,  785,  786,  787,  788,  789,  790,  790,  791,  792,  793,  794,  795, \
     795,  796,  797,  798,  799,  800,  801,  801,  802,  803,  804,  805,  806,  807,  807,  808, \
     809,  810,  811,  812,  813,  813,  814,  815,  816,  817,  818,  819,  819,  820,  821,  822, \
     823,  824,  825,  825,  826,  827,  828,  829,  830,  831,  832,  832,  833,  834,  835,  836, \
     837,  838,  839,  839,  840,  841,  842,  843,  844,  845,  846,  846,  847,  848,  849,  850, \
     851,  852,  853,  854,  854,  855,  856,  857,  858,  859,  860,  861,  862,  862,  863,  864, \
     865,  866,  867,  868,  869,  870,  871,  871,  872,  873,  874,  875,  876,  877,  878,  879, \
     880,  880,  881,  882,  883,  884,  885,  886,  887,  888,  889,  890,  890,  891,  892,  893, \
     894,  895,  896,  897,  898,  899,  900,  901,  901,  902,  903,  904,  905,  906,  907,  908, \
     909,  910,  911,  912,  913,  914,  914,  915,  916,  917,  918,  919,  920,  921,  922,  923, \
     924,  925,  926,  927,  928,  929,  930,  930,  931,  932,  933,  934,  935,  936,  937,  938, \
     939,  940,  941,  942,  943,  944,  945,  946,  947,  948,  949,  950,  951,  952,  952,  953, \
     954,  955,  956,  957,  958,  959,  960,  961,  962,  963,  964,  965,  966,  967,  968,  969, \
     970,  971,  972,  973,  974,  975,  976,  977,  978,  979,  980,  981,  982,  983,  984,  985, \
     986,  987,  988,  989,  990,  991,  992,  993,  994,  995,  996,  997,  998,  999, 1000, 1001, \
    1002, 1003, 1004, 1005, 1006, 1007, 1008, 1009, 1010, 1011, 1012, 1013, 1014, 1015, 1016, 1017, \
    1018, 1019, 1020, 1021, 1022, 1023, 1024, 1025, 1026, 1027, 1029, 1030, 1031, 1032, 1033, 1034, \
    1035, 1036, 1037, 1038, 1039, 1040, 1041, 1042, 1043, 1044, 1045, 1046, 1047, 1048, 1049, 1051, \
    1052, 1053, 1054, 1055, 1056, 1057, 1058, 1059, 1060, 1061, 1062, 1063, 1064, 1065, 1067, 1068, \
    1069, 1070, 1071, 1072, 1073, 1074, 1075, 1076, 1077, 1079, 1080, 1081, 1082, 1083, 1084, 1085, \
    1086, 1087, 1088, 1089, 1091, 1092, 1093, 1094, 1095, 1096, 1097, 1098, 1099, 1101, 1102, 1103, \
    1104, 1105, 1106, 1107, 1108, 1110, 1111, 1112, 1113, 1114, 1115, 1116, 1117, 1119, 1120, 1121, \
    1122, 1123, 1124, 1125, 1127, 1128, 1129, 1130, 1131, 1132, 1134, 1135, 1136, 1137, 1138, 1139, \
    1140, 1142, 1143, 1144, 1145, 1146, 1148, 1149, 1150, 1151, 1152, 1153, 1155, 1156, 1157, 1158, \
    1159, 1161, 1162, 1163, 1164, 1165, 1166, 1168, 1169, 1170, 1171, 1173, 1174, 1175, 1176, 1177, \
    1179, 1180, 1181, 1182, 1183, 1185, 1186, 1187, 1188, 1190, 1191, 1192, 1193, 1195, 1196, 1197, \
    1198, 1199, 1201, 1202, 1203, 1204, 1206, 1207, 1208, 1209, 1211, 1212, 1213, 1215, 1216, 1217, \
    1218, 1220, 1221, 1222, 1223, 1225, 1226, 1227, 1229, 1230, 1231, 1232, 1234, 1235, 1236, 1238, \
    1239, 1240, 1242, 1243, 1244, 1245, 1247, 1248, 1249, 1251, 1252, 1253, 1255, 1256, 1257, 1259, \
    1260, 1261, 1263, 1264, 1265, 1267, 1268, 1269, 1271, 1272, 1274, 1275, 1276, 1278, 1279, 1280, \
    1282, 1283, 1284, 1286, 1287, 1289, 1290, 1291, 1293, 1294, 1296, 1297, 1298, 1300, 1301, 1303, \
    1304, 1305, 1307, 1308, 1310, 1311, 1312, 1314, 1315, 1317, 1318, 1320, 1321, 1322, 1324, 1325, \
    1327, 1328, 1330, 1331, 1333, 1334, 1336, 1337, 1339, 1340, 1341, 1343, 1344, 1346, 1347, 1349, \
    1350, 1352, 1353, 1355, 1356, 1358, 1359, 1361, 1362, 1364, 1365, 1367, 1369, 1370, 1372, 1373, \
    1375, 1376, 1378, 1379, 1381, 1382, 1384, 1386, 1387, 1389, 1390, 1392, 1393, 1395, 1397, 1398, \
    1400, 1401, 1403, 1405, 1406, 1408, 1409, 1411, 1413, 1414, 1416, 1418, 1419, 1421, 1422, 1424, \
    1426, 1427, 1429, 1431, 1432, 1434, 1436, 1437, 1439, 1441, 1442, 1444, 1446, 1448, 1449, 1451, \
    1453, 1454, 1456, 1458, 1460, 1461, 1463, 1465, 1467, 1468, 1470, 1472, 1474, 1475, 1477, 1479, \
    1481, 1482, 1484, 1486, 1488, 1490, 1491, 1493, 1495, 1497, 1499, 1501, 1502, 1504, 1506, 1508, \
    1510, 1512, 1513, 1515, 1517, 1519, 1521, 1523, 1525, 1527, 1529, 1531, 1532, 1534, 1536, 1538, \
    1540, 1542, 1544, 1546, 1548, 1550, 1552, 1554, 1556, 1558, 1560, 1562, 1564, 1566, 1568, 1570, \
    1572, 1574, 1576, 1578, 1580, 1582, 1584, 1586, 1588, 1591, 1593, 1595, 1597, 1599, 1601, 1603, \
    1605, 1608, 1610, 1612, 1614, 1616, 1618, 1621, 1623, 1625, 1627, 1629, 1632, 1634, 1636, 1638, \
    1641, 1643, 1645, 1647, 1650, 1652, 1654, 1657, 1659, 1661, 1664, 1666, 1668, 1671, 1673, 1675, \
    1678, 1680, 1683, 1685, 1687, 1690, 1692, 1695, 1697, 1700, 1702, 1705, 1707, 1710, 1712, 1715, \
    1717, 1720, 1723, 1725, 1728, 1730, 1733, 1736, 1738, 1741, 1744, 1746, 1749, 1752, 1754, 1757, \
    1760, 1763, 1765, 1768, 1771, 1774, 1777, 1779, 1782, 1785, 1788, 1791, 1794, 1797, 1800, 1802, \
    1805, 1808, 1811, 1814, 1817, 1820, 1824, 1827, 1830, 1833, 1836, 1839, 1842, 1845, 1849, 1852, \
    1855, 1858, 1861, 1865, 1868, 1871, 1875, 1878, 1881, 1885, 1888, 1892, 1895, 1899, 1902, 1906, \
    1909, 1913, 1916, 1920, 1924, 1927, 1931, 1935, 1938, 1942, 1946, 1950, 1954, 1958, 1962, 1965, \
    1969, 1973, 1977, 1982, 1986, 1990, 1994, 1998, 2002, 2007, 2011, 2015, 2020, 2024, 2028, 2033, \
    2037, 2042, 2047, 2051, 2056, 2061, 2065, 2070, 2075, 2080, 2085, 2090, 2095, 2100, 2105, 2110, \
    2116, 2121, 2126, 2132, 2137, 2143, 2149, 2154, 2160, 2166, 2172, 2178, 2184, 2190, 2196, 2202, \
    2209, 2215, 2222, 2228, 2235, 2242, 2249, 2256, 2263, 2270, 2278, 2285, 2293, 2301, 2309, 2317, \
    2325, 2333, 2342, 2350, 2359, 2368, 2377, 2387, 2396, 2406, 2416, 2426, 2437, 2447, 2458, 2470, \
    2481, 2493, 2506, 2518, 2532, 2545, 2559, 2574, 2589, 2604, 2620, 2637, 2655, 2673, 2693, 2713, \
    2735, 2758, 2782, 2808, 2836, 2866, 2899, 2935, 2976, 3021, 3074, 3136, 3212, 3312, 3458, 3756
// ---- end generated ----
// clang-format on

namespace sd {

constexpr int NOISE_T = 256, NOISE_STEPS = 8, NOISE_UNROLL = 4;          // threads of a block, chunks of a thread, chunks it has in flight
constexpr int NOISE_STRIP_CHUNKS = NOISE_T * NOISE_STEPS;
constexpr int64_t NOISE_STRIP_BYTES = (int64_t)NOISE_STRIP_CHUNKS * 16;
constexpr uint32_t NOISE_MAX_A = 1u << 26, NOISE_MAX_B = 1u << 17;       // the clamps of the row's variance words

static const uint16_t h_noise_half[2048] = {SD_NOISE_HALF_TABLE};                        // the host's copy: sd_noise_normal_table
__device__ __align__(16) const uint16_t d_noise_half[2048] = {SD_NOISE_HALF_TABLE};

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t k0, uint32_t k1, uint32_t r[4]) {
    uint32_t x0 = c0, x1 = 0, x2 = 0, x3 = 0;
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * x0, p1 = (uint64_t)0xCD9E8D57u * x2;   // one v_mad_u64_u32 each: both halves
        x0 = (uint32_t)(p1 >> 32) ^ x1 ^ k0;
        x1 = (uint32_t)p1;
        x2 = (uint32_t)(p0 >> 32) ^ x3 ^ k1;
        x3 = (uint32_t)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    r[0] = x0, r[1] = x1, r[2] = x2, r[3] = x3;
}

// floor(sqrt(x)), x < 2^27: the float root is within 1 of it
__device__ __forceinline__ uint32_t noise_isqrt(uint32_t x) {
    uint32_t s = (uint32_t)sqrtf((float)x);
    if (s * s > x) --s;
    if ((s + 1) * (s + 1) <= x) ++s;
    return s;
}

__device__ __forceinline__ uint32_t noise_byte(uint32_t v, uint32_t word, const uint16_t* half, const uint16_t* sigma) {
    const int i = (int)(word >> 20);
    const int mag = half[i >= 2048 ? i - 2048 : 2047 - i];
    const int z = i >= 2048 ? mag : -mag;
    const int n = (z * (int)sigma[v] + (1 << 17)) >> 18;
    return (uint32_t)min(max((int)v + n, 0), 255);
}

// the four bytes of the dword w are the bytes 4 g .. 4 g + 3 of the image: one call
__device__ __forceinline__ uint32_t noise_dword(uint32_t w, uint32_t g, uint32_t k0, uint32_t k1, const uint16_t* half, const uint16_t* sigma) {
    uint32_t r[4];
    philox4x32_10(g, k0, k1, r);
    uint32_t y = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) y |= noise_byte((w >> (8 * j)) & 255u, r[j], half, sigma) << (8 * j);
    return y;
}

template <bool VEC>
__device__ __forceinline__ uint4 noise_load(const uint8_t* p) {
    if (VEC) return *reinterpret_cast<const uint4*>(p);
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 16; ++k) w[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

template <bool VEC>
__device__ __forceinline__ void noise_store(uint8_t* p, const uint4& v) {
    if (VEC) {
        *reinterpret_cast<uint4*>(p) = v;
        return;
    }
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 16; ++k) p[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
}

// the block's whole chunks: c0 = the image's chunk index of the block's first one, mine of them (<= NOISE_STRIP_CHUNKS)
template <bool VEC>
__device__ __forceinline__ void noise_strip(const uint8_t* img, uint8_t* dst, int64_t c0, int mine, bool on, uint32_t k0, uint32_t k1,
                                            const uint16_t* half, const uint16_t* sigma) {
    const int tid = threadIdx.x;
    for (int base = tid; base < mine; base += NOISE_T * NOISE_UNROLL) {
        uint4 v[NOISE_UNROLL];
#pragma unroll
        for (int u = 0; u < NOISE_UNROLL; ++u)
            if (base + NOISE_T * u < mine) v[u] = noise_load<VEC>(img + 16 * (c0 + base + NOISE_T * u));
#pragma unroll
        for (int u = 0; u < NOISE_UNROLL; ++u)
            if (base + NOISE_T * u < mine) {
                const int64_t c = c0 + base + NOISE_T * u;
                if (on) {
                    const uint32_t g = (uint32_t)(4 * c);                // 4 c + 3 < 3 H W / 4 < 2^31
                    v[u].x = noise_dword(v[u].x, g, k0, k1, half, sigma);
                    v[u].y = noise_dword(v[u].y, g + 1, k0, k1, half, sigma);
                    v[u].z = noise_dword(v[u].z, g + 2, k0, k1, half, sigma);
                    v[u].w = noise_dword(v[u].w, g + 3, k0, k1, half, sigma);
                }
                noise_store<VEC>(dst + 16 * c, v[u]);
            }
    }
}

__global__ __launch_bounds__(NOISE_T) void k_noise_u8(const uint8_t* in, uint8_t* out, int64_t nb, const int* __restrict__ table) {
    const int b = blockIdx.y;
    const uint32_t k0 = (uint32_t)table[4 * b], k1 = (uint32_t)table[4 * b + 1];
    const uint32_t a = min((uint32_t)table[4 * b + 2], NOISE_MAX_A), g = min((uint32_t)table[4 * b + 3], NOISE_MAX_B);
    const bool on = (a | g) != 0;
    if (!on && in == out) return;                                        // uniform per block: the identity in place touches no memory
    __shared__ __align__(16) uint16_t s_half[2048];
    __shared__ uint16_t s_sigma[256];
    const int tid = threadIdx.x;
    if (on) {
        reinterpret_cast<uint4*>(s_half)[tid] = reinterpret_cast<const uint4*>(d_noise_half)[tid];   // 256 threads x 8 entries
        s_sigma[tid] = (uint16_t)noise_isqrt(a + g * (uint32_t)tid);     // <= 2^26 + 255 * 2^17 < 2^27: a root below 10027
    }
    __syncthreads();
    const uint8_t* img = in + b * nb;
    uint8_t* dst = out + b * nb;
    const int64_t chunks = nb >> 4;
    const int64_t c0 = (int64_t)blockIdx.x * NOISE_STRIP_CHUNKS;
    const int mine = (int)max((int64_t)0, min((int64_t)NOISE_STRIP_CHUNKS, chunks - c0));
    if (((reinterpret_cast<uintptr_t>(img) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0)
        noise_strip<true>(img, dst, c0, mine, on, k0, k1, s_half, s_sigma);
    else
        noise_strip<false>(img, dst, c0, mine, on, k0, k1, s_half, s_sigma);
    if (blockIdx.x == gridDim.x - 1) {                                   // the bytes behind the last whole chunk
        const int64_t o = 16 * chunks + tid;
        if (o < nb) {
            uint32_t v = img[o];
            if (on) {
                uint32_t r[4];
                philox4x32_10((uint32_t)(o >> 2), k0, k1, r);
                const int j = (int)(o & 3);
                v = noise_byte(v, j == 0 ? r[0] : j == 1 ? r[1] : j == 2 ? r[2] : r[3], s_half, s_sigma);
            }
            dst[o] = (uint8_t)v;
        }
    }
}

// in -> out, (B, H, W, 3) u8, out == in allowed (no other overlap).  Shapes and pointers are the caller's to check (B is a grid
// dimension: <= 65535; H W < 2^31).
int noise_stage(const uint8_t* in, uint8_t* out, int B, int H, int W, const int* table, hipStream_t st) {
    const int64_t nb = 3 * (int64_t)H * W;
    const dim3 grid(cdiv(nb, NOISE_STRIP_BYTES), B);                     // < 3 * 2^31 / 2^15 blocks; the last one owns the tail
    hipLaunchKernelGGL(k_noise_u8, grid, dim3(NOISE_T), 0, st, in, out, nb, table);
    SD_LAUNCH_CHECK();
    return 0;
}

}  // namespace sd

using namespace sd;

extern "C" {

int sd_noise_normal_table(uint16_t* out) {
    SD_REQUIRE(out, SD_ERR_INVALID, "sd_noise_normal_table: null pointer");
    for (int j = 0; j < 2048; ++j) out[j] = h_noise_half[j];
    return 0;
}

int sd_noise_u8(const uint8_t* in, uint8_t* out, int B, int H, int W, const int* table, sd_stream_t stream) {
    SD_REQUIRE(in && out && table, SD_ERR_INVALID, "sd_noise_u8: null pointer");
    SD_REQUIRE(B > 0 && H > 0 && W > 0, SD_ERR_INVALID, "sd_noise_u8: bad shape");
    SD_REQUIRE(B <= 65535 && (int64_t)H * W < (1ll << 31), SD_ERR_INVALID, "sd_noise_u8: batch %d > 65535 or %d x %d >= 2^31 pixels", B, W, H);
    const int64_t bytes = (int64_t)B * H * W * 3;
    SD_REQUIRE(in == out || in + bytes <= out || out + bytes <= in, SD_ERR_INVALID, "sd_noise_u8: out must be in or not overlap it");
    return noise_stage(in, out, B, H, W, table, (hipStream_t)stream);
}

}  // extern "C"
