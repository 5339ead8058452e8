"""Known answers the oracle's golden tests and the GPU parity tests share."""
SURVEY_KAT_CASE0 = [  # test case 0, ORCA robot, robot invisible — an INDEPENDENT float32 restatement
    ((-0.051465511322021484, 0.45335352420806885),
     '7424d63eb76eca3e 54b22d3f3cac3d3c 8e4c2cbf7e45a4bd cef9a9be10f4113f 100e253ff8dc75be'),
    ((0.08838461339473724, 0.512067437171936),
     '937cd13e6ac1e13e d51f243f9bd3923c ea9c24bf57a289bd b972adbe7e250a3f e88f313f5b7393be'),
    ((0.07480747997760773, 0.5604285597801208),
     'ff69c03e5c7df23e c2471a3fb26bff3c efb71dbfd3e653bd f3b4a1be45cd053f 8fbd533fe931aabe'),
]
